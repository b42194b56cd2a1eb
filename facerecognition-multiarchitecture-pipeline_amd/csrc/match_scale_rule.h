// The power-of-two row scale of the split-fp16 matcher (head_match.hip: match_row_prep_kernel, match_pack_gallery_kernel), for the
// host and the device alike: the kernels run this text and a plain C++ compiler takes it too (tools/match_scale_check.cpp sweeps it
// over every fp32 exponent).  Not part of the public ABI.
//
// A row x with amax = max |x_k| is split as hi = fp16(S x), lo = fp16(S x - hi) and its statistics carry 1 / S, which the match
// GEMM's epilogue multiplies the scaled dot product by and the gallery packer inverts again to get S back.  So for EVERY fp32 amax
//   * S is a finite positive power of two, and so is 1 / S, which is moreover NORMAL (biased exponent 1 .. 254, mantissa 0):
//     1 / (1 / S) == S bit for bit whatever the denormal mode of the device, and neither is ever 0, inf or NaN;
//   * amax S < 2^14 <= 65504: nothing overflows fp16;
//   * amax >= FRMAP_MATCH_SCALE_CUT = 2^-113: amax S lies in [2^13, 2^14), so lo stays out of the fp16 subnormals for every element
//     within 2^-11 of the row maximum.
// The exponent is CLAMPED below the cut (S = 2^126, 1 / S = 2^-126, the smallest normal): an unclamped 2^(14 - e) is 2^127 with a
// subnormal inverse at e = -113 and +inf from e = -114 down, which turned such a row into inf and NaN on both sides of the GEMM.
// Why the clamp is safe.  Below the cut S x < 2^13, and the pair (hi, lo) holds S x to within max(2^-22 |S x|, 2^-25) (2^-25 = half
// the spacing of the fp16 subnormals, where lo ends up once it has lost all of its bits): x itself to within 2^-151, less than half
// the smallest fp32 subnormal.  That absolute part moves the dot product with any row g by at most 2^-151 sum |g_k| <= 2^-151
// sqrt(K) |g|, while the bound the epilogue already allows, kappa (band(a) + band(g) + K eps^2) (match_device.h), is at least
// 2^-18 * 2 eps sqrt(K) |g| > 2^-38 sqrt(K) |g|: 2^113 times more.  The relative part is that of every other row.
// A zero row, and a row whose maximum is an infinity (or which holds nothing but NaN), keeps S = 1.
// Integer arithmetic on the bits throughout: no frexp / ldexp whose treatment of subnormals could differ between the two sides.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRMAP_MATCH_HD __host__ __device__
#else
#define FRMAP_MATCH_HD
#endif

constexpr int FRMAP_MATCH_SCALE_CUT_EXP = -113;   // the cut is 2^-113: below it the exponent of S is clamped (S = 2^126)

// amax: the largest |x_k| of the row (>= 0, or NaN)
FRMAP_MATCH_HD inline float frmap_match_row_scale(float amax) {
  uint32_t bits;
  __builtin_memcpy(&bits, &amax, 4);
  int be = (int)((bits >> 23) & 0xFFu);                     // amax in [2^(be - 127), 2^(be - 126)) for be >= 1
  if ((bits << 1) == 0u || be == 255) return 1.f;           // zero; inf / NaN
  const int be_cut = FRMAP_MATCH_SCALE_CUT_EXP + 127;       // 14
  if (be < be_cut) be = be_cut;                             // (subnormals: be = 0)
  const uint32_t sbits = (uint32_t)(127 + 13 + 127 - be) << 23;   // S = 2^(13 - (be - 127)): biased exponent 13 .. 253
  float S;
  __builtin_memcpy(&S, &sbits, 4);
  return S;
}
