// The split-fp16 matcher's row scale (csrc/match_scale_rule.h, nothing else of the kernels) as a stand-alone program, for a build
// with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/match_scale_check.cpp -o check && ./check
// It sweeps every fp32 exponent from -149 to 127 - the subnormals bit by bit, every normal binade - with the mantissa at its lowest,
// a middle and its highest value, and checks for each amax what the header promises:
//   * S is a finite, positive power of two;
//   * 1 / S is finite, nonzero and NORMAL (mantissa field 0, biased exponent 1 .. 254): nothing rests on a denormal mode;
//   * 1 / (1 / S) == S bit for bit;
//   * amax S <= 65504 (the largest fp16);
//   * amax S lies in [2^13, 2^14) for every amax >= the cut 2^FRMAP_MATCH_SCALE_CUT_EXP, and the cut is the lowest such exponent;
//   * a zero row, an infinity and a NaN keep S = 1.
// Exit status 0 and "self check passed" on success.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "match_scale_rule.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAILED %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

static uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
static float float_of(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static bool normal_power_of_two(float f) {
  const uint32_t b = bits_of(f), be = (b >> 23) & 0xFFu;
  return (b >> 31) == 0u && (b & 0x7FFFFFu) == 0u && be >= 1u && be <= 254u;
}

static int checked = 0;
static bool below_cut_seen = false;

// e: amax lies in [2^e, 2^(e + 1))
static void check_one(float amax, int e) {
  const volatile float S = frmap_match_row_scale(amax);
  const volatile float inv = 1.0f / S;
  const volatile float back = 1.0f / inv;
  const volatile float top = amax * S;
  CHECK(normal_power_of_two(S), "amax=%a (2^%d): S=%a", (double)amax, e, (double)S);
  CHECK(normal_power_of_two(inv), "amax=%a (2^%d): 1/S=%a is not a normal power of two", (double)amax, e, (double)inv);
  CHECK(bits_of(back) == bits_of(S), "amax=%a (2^%d): 1/(1/S)=%a != S=%a", (double)amax, e, (double)back, (double)S);
  CHECK(top <= 65504.0f, "amax=%a (2^%d): amax S = %a overflows fp16", (double)amax, e, (double)top);
  if (e >= FRMAP_MATCH_SCALE_CUT_EXP) {
    CHECK(top >= 8192.0f && top < 16384.0f, "amax=%a (2^%d): amax S = %a outside [2^13, 2^14)", (double)amax, e, (double)top);
  } else {
    CHECK(top < 8192.0f, "amax=%a (2^%d) lies below the cut, yet amax S = %a", (double)amax, e, (double)top);
    CHECK(bits_of(S) == bits_of(ldexpf(1.0f, 126)), "amax=%a (2^%d): S=%a below the cut is not 2^126", (double)amax, e, (double)S);
    below_cut_seen = true;
  }
  ++checked;
}

int main() {
  for (int e = -149; e <= 127; ++e) {
    uint32_t lo, mid, hi;
    if (e < -126) {                         // subnormals: the leading bit at position e + 149, the bits below it free
      const uint32_t lead = 1u << (e + 149);
      lo = lead; mid = lead | (lead >> 1); hi = lead | (lead - 1u);
    } else {
      const uint32_t be = (uint32_t)(e + 127) << 23;
      lo = be; mid = be | 0x400000u; hi = be | 0x7FFFFFu;
    }
    const uint32_t m[3] = {lo, mid, hi};
    for (int i = 0; i < 3; ++i) {
      const float amax = float_of(m[i]);
      CHECK(amax > 0.0f && amax >= ldexpf(1.0f, e) && (e == 127 || amax < ldexpf(1.0f, e + 1)), "the sweep itself: %a at 2^%d", (double)amax, e);
      check_one(amax, e);
    }
  }
  CHECK(checked == 3 * 277, "swept %d values", checked);
  CHECK(below_cut_seen && FRMAP_MATCH_SCALE_CUT_EXP == -113, "the cut moved: say so in the header, the rule file and here");
  CHECK(frmap_match_row_scale(0.0f) == 1.0f && frmap_match_row_scale(-0.0f) == 1.0f, "a zero row keeps S = 1");
  CHECK(frmap_match_row_scale(INFINITY) == 1.0f && frmap_match_row_scale(NAN) == 1.0f, "an inf / NaN maximum keeps S = 1");
  printf("self check passed: %d values, cut 2^%d\n", checked, FRMAP_MATCH_SCALE_CUT_EXP);
  return 0;
}
