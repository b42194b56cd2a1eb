// A pixel as R | G << 8 | B << 16, for the host and the device alike: packing, the 3-byte store, the read of a packed frame, and
// THE warp - pixel (x, y) of Pillow's Image.rotate output (Geometry.c: affine_transform + bilinear_filter32RGB), written once
// for every source of pixels.  The crop kernels (crop_device.h) call it where a filter tap reads a rotated pixel; the host twins
// (frmap_align_warp_host, frmap_yuv_align_warp_twin) run the same text on the CPU, and tools/yuv_check.cpp includes it under a
// plain C++ compiler with the sanitizers.  Not part of the public ABI.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRMAP_HD __host__ __device__
#else
#define FRMAP_HD
#endif

FRMAP_HD inline unsigned frmap_rgb_pack(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }

FRMAP_HD inline void frmap_rgb_store3(unsigned char* o, unsigned v) {
  o[0] = (unsigned char)(v & 255u); o[1] = (unsigned char)((v >> 8) & 255u); o[2] = (unsigned char)((v >> 16) & 255u);
}

// Pixel (x, y) of a packed frame (3 bytes per pixel, `pitch` bytes per row; c0 = the byte of a pixel that holds R: 0, or 2 for
// BGR frames), 0 <= x < W, 0 <= y < H.  Offsets in 64 bits.
struct FrmapPackedFetch {
  const unsigned char* base;
  long long pitch;
  int c0;
  FRMAP_HD unsigned operator()(int x, int y) const {
    const unsigned char* p = base + (size_t)y * pitch + (size_t)x * 3;
    return frmap_rgb_pack(p[c0], p[1], p[2 - c0]);
  }
};

// Pixel (x, y) of Image.rotate's output for an H x W frame whose pixels `fetch(x, y)` returns, and the output -> input matrix
// m[6] (the host's: frames.rotation_matrix; Pillow rounds cos / sin to 15 DECIMALS, which only decimal arithmetic reproduces).
// The four corners are uint8 RGB before the float64 arithmetic touches them and the result is truncated to 8 bits, because Pillow
// resizes the uint8 image that rotate() returned.  Every index is clamped to the frame and a sample outside it (NaN coordinates
// included: the test is written so that NaN fails it) is 0, so nothing is fetched outside the frame whatever the matrix holds.
// As in resize_coeffs.h the operation order is Pillow's and nothing may be fused into an FMA, so contraction is off.
template <class Fetch>
FRMAP_HD inline unsigned frmap_warp_pixel(int H, int W, const double* m, int x, int y, const Fetch& fetch) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xo = x + 0.5, yo = y + 0.5;
  double xin = m[0] * xo + m[1] * yo + m[2];
  double yin = m[3] * xo + m[4] * yo + m[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return 0u;
  xin -= 0.5;
  yin -= 0.5;
  const int xi = (int)floor(xin), yi = (int)floor(yin);          // in [-1, W - 1] x [-1, H - 1]
  const double dx = xin - xi, dy = yin - yi;
  const int xa = xi < 0 ? 0 : xi, xb = xi + 1 < W ? xi + 1 : W - 1, ya = yi < 0 ? 0 : yi;
  const bool below = yi + 1 < H;                                 // (yi + 1 >= 0 always)
  const unsigned p00 = fetch(xa, ya), p01 = fetch(xb, ya);
  unsigned p10 = 0u, p11 = 0u;
  if (below) {
    p10 = fetch(xa, yi + 1);
    p11 = fetch(xb, yi + 1);
  }
  unsigned out = 0u;
  for (int c = 0; c < 3; ++c) {
    const int a0 = (int)((p00 >> (8 * c)) & 255u), a1 = (int)((p01 >> (8 * c)) & 255u);
    const double v1 = a0 + (a1 - a0) * dx;
    double v2 = v1;
    if (below) {
      const int b0 = (int)((p10 >> (8 * c)) & 255u), b1 = (int)((p11 >> (8 * c)) & 255u);
      v2 = b0 + (b1 - b0) * dx;
    }
    out |= (unsigned)(int)(v1 + (v2 - v1) * dy) << (8 * c);       // (UINT8) of a value in [0, 255]: truncation
  }
  return out;
}
