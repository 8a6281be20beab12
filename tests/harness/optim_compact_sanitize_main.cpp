/* Stand-alone program over csrc/prl_optim_sr.h and the host harness of the compact optimizer step, to be built with
 * -fsanitize=address,undefined and run on its own (tests/test_optim_compact_host.py does): the known answers of the generator,
 * the rounding of the edge values under every random value, and compact AdamW / Lion steps in every mode on heap arrays of
 * exactly n elements, so that an access past an end or an undefined shift is reported.  Test-only. */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "optim_compact_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "FAILED: %s\n", what);
  return 1;
}

int main() {
  const uint32_t counters[3][4] = {{0, 0, 0, 0}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
  const uint32_t keys[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
  const uint32_t want[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
                               {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                               {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
  for (int k = 0; k < 3; ++k) {
    uint32_t out[4];
    prl_host_philox4x32_10(counters[k], keys[k], out);
    for (int j = 0; j < 4; ++j)
      if (out[j] != want[k][j]) return fail("known answer");
  }
  const uint32_t edge_bits[] = {0x3f800001u, 0x00000001u, 0xbf80ffffu, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0x80000000u, 0u};
  std::vector<uint16_t> all(65536);
  for (uint32_t u : edge_bits) {
    float f;
    memcpy(&f, &u, 4);
    prl_host_sr_all(f, all.data());
    long up = 0;
    for (uint32_t r = 0; r < 65536u; ++r) up += all[r] != (uint16_t)(u >> 16);
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
    if (!nan && up != (long)(u & 0xffffu)) return fail("count of values rounded up");
  }
  const long sizes[] = {1, 3, 4, 5, 8, 1003};
  for (long n : sizes)
    for (int mode = 0; mode < 4; ++mode)
      for (int sb = 0; sb < 2; ++sb) {
        std::vector<float> g(n), master(n, 0.25f);
        for (long i = 0; i < n; ++i) g[i] = 1e-3f * (float)(i % 17 - 8);
        const size_t pe = mode == 0 ? 4 : 2, se = sb ? 2 : 4;
        void* p = calloc(n, pe);
        void* m = calloc(n, se);
        void* v = calloc(n, se);
        for (long step = 1; step <= 3; ++step) {
          prl_host_compact_adamw(n, 1e-3, 0.01, 0.9, 0.999, 1e-8, step, 0.5f, g.data(), p, mode == 1 ? master.data() : nullptr, m, v, mode, sb,
                                 (1L << 40) + 4, 0xffffffffL, 0xffffffffffffffffull);
          prl_host_compact_lion(n, 1e-4, 0.01, 0.9, 0.99, step, 1.0f, g.data(), p, mode == 1 ? master.data() : nullptr, m, mode, sb, 16, 3, 12345);
        }
        free(p);
        free(m);
        free(v);
      }
  printf("ok\n");
  return 0;
}
