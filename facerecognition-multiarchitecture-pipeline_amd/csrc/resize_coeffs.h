// Pillow's bilinear filter taps for one axis (libImaging/Resample.c: precompute_coeffs with the bilinear filter, support 1, box =
// the whole axis, then normalize_coeffs_8bpc), one output sample at a time, for the host and the device alike: the crop body
// (crop_device.h) builds its tables with it in LDS and frmap_resize_coeffs_host runs the same text on the CPU.  At the end, the
// integer sum of one output sample that both resize kernels (resize.hip, crop_device.h) run over those taps.  Not part of the
// public ABI.
//
// The integers must equal Pillow's, so the float64 operation order is Pillow's and nothing may be fused: hipcc contracts a * b + c
// into an FMA on the device by default, and `center = (xx + 0.5) * scale` followed by `center - support + 0.5` then rounds
// differently from the C code.  Every function below therefore turns contraction off; division stays the correctly rounded
// default (the library is not built with fast-math).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "rgb_pixel.h"

constexpr int FRMAP_RESIZE_PRECISION_BITS = 32 - 8 - 2;

struct FrmapResizeAxis {
  double scale, support, ss;
  int in_size;
  int ksize;   // taps per output sample, ceil(support) * 2 + 1 (Pillow's table pitch)
};

__host__ __device__ inline FrmapResizeAxis frmap_resize_axis(int in_size, int out_size) {
#pragma clang fp contract(off)
  FrmapResizeAxis a;
  double filterscale = a.scale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  a.support = 1.0 * filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  a.ss = 1.0 / filterscale;
  a.in_size = in_size;
  return a;
}

// the un-normalised weight of tap x of the sample centred at `center`: bilinear_filter((x + xmin - center + 0.5) * ss)
__host__ __device__ inline double frmap_resize_weight(const FrmapResizeAxis& a, double center, int xmin, int x) {
#pragma clang fp contract(off)
  double v = (x + xmin - center + 0.5) * a.ss;
  if (v < 0.0) v = -v;
  return v < 1.0 ? 1.0 - v : 0.0;
}

// Output sample xx: *first = the first input sample it reads, *taps = how many (<= a.ksize), k[0 .. *taps) = the 22-bit integer
// coefficients (weights summed left to right, each divided by the sum, scaled by 2^22, rounded half away from zero by a truncating
// cast).  The weights are evaluated twice - once for the sum, once for the quotients - so no per-sample array is needed; the two
// evaluations are the same operations on the same operands.
__host__ __device__ inline void frmap_resize_taps(const FrmapResizeAxis& a, int xx, int* first, int* taps, int* k) {
#pragma clang fp contract(off)
  const double center = 0.0 + (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > a.in_size) xmax = a.in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += frmap_resize_weight(a, center, xmin, x);
  for (int x = 0; x < xmax; ++x) {
    double w = frmap_resize_weight(a, center, xmin, x);
    if (ww != 0.0) w /= ww;
    const double p = w * (double)(1 << FRMAP_RESIZE_PRECISION_BITS);
    k[x] = w < 0 ? (int)(-0.5 + p) : (int)(0.5 + p);
  }
  *first = xmin;
  *taps = xmax;
}

// One output sample of Resample.c's horizontal or vertical 8-bit pass: three int32 sums started at half an output
// unit, a tap adds pixel * coefficient per channel, the result is shifted (arithmetic) and clipped to [0, 255].
struct FrmapResizeSum {
  int s0 = 1 << (FRMAP_RESIZE_PRECISION_BITS - 1), s1 = 1 << (FRMAP_RESIZE_PRECISION_BITS - 1), s2 = 1 << (FRMAP_RESIZE_PRECISION_BITS - 1);
  __device__ __forceinline__ void tap(unsigned t, int w) {   // t = R | G << 8 | B << 16
    s0 += (int)(t & 255u) * w; s1 += (int)((t >> 8) & 255u) * w; s2 += (int)((t >> 16) & 255u) * w;
  }
  static __device__ __forceinline__ unsigned clip8(int v) {
    v >>= FRMAP_RESIZE_PRECISION_BITS;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
  __device__ __forceinline__ unsigned pixel() const { return frmap_rgb_pack(clip8(s0), clip8(s1), clip8(s2)); }
};
