// One pixel of a 4:2:0 YUV frame as RGB, for the host and the device alike: the YUV crop kernels (yuv_crop.hip) convert a
// filter tap's pixel where the tap reads it, so no RGB frame is ever written; frmap_yuv_to_rgb_host / frmap_yuv_align_warp_host
// run the same text on the CPU and tools/yuv_check.cpp includes it under a plain C++ compiler with the sanitizers.  Not part of
// the public ABI.
//
// THE RULE ("YUV frames").  Chroma: pixel (x, y) takes chroma sample (x >> 1, y >> 1) - nearest replication,
// no interpolation; the chroma planes are ceil(H/2) x ceil(W/2).  Colour: 16-bit fixed point in int32, every coefficient
// floor(c * 65536 + 0.5) of its float64 value derived from (Kr, Kb) and the range's scaling,
//     R = clip8((cy (Y - y_off) + rv (V - 128) + 32768) >> 16)
//     G = clip8((cy (Y - y_off) + gu (U - 128) + gv (V - 128) + 32768) >> 16)
//     B = clip8((cy (Y - y_off) + bu (U - 128) + 32768) >> 16)
// with an arithmetic shift; |sum| < 3.6e7.  The pixel is uint8 RGB BEFORE anything else touches it: a crop of a YUV frame is the
// crop of the converted frame, bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>

#include "frame_records.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRMAP_YUV_HD __host__ __device__
#else
#define FRMAP_YUV_HD
#endif

constexpr int FRMAP_YUV_CSC_COUNT = 4;

struct FrmapYuvCsc {
  int y_off, cy, rv, gu, gv, bu;
};

// row `csc` of the table (frames.YUV_COEFFS); csc outside [0, 4) is the caller's to refuse
FRMAP_YUV_HD inline FrmapYuvCsc frmap_yuv_csc(int csc) {
  switch (csc) {
    case 0: return FrmapYuvCsc{16, 76309, 104597, -25675, -53279, 132201};    // bt601, limited
    case 1: return FrmapYuvCsc{0, 65536, 91881, -22553, -46802, 116130};      // bt601, full
    case 2: return FrmapYuvCsc{16, 76309, 117489, -13975, -34925, 138438};    // bt709, limited
    default: return FrmapYuvCsc{0, 65536, 103206, -12276, -30679, 121609};    // bt709, full
  }
}

FRMAP_YUV_HD inline int frmap_yuv_clip8(int v) {
  v >>= 16;                                                                   // arithmetic: v may be negative
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (Y, U, V) -> R | G << 8 | B << 16
FRMAP_YUV_HD inline unsigned frmap_yuv_rgb(int Y, int U, int V, const FrmapYuvCsc& k) {
  const int l = k.cy * (Y - k.y_off) + 32768, u = U - 128, v = V - 128;
  return (unsigned)frmap_yuv_clip8(l + k.rv * v) | ((unsigned)frmap_yuv_clip8(l + k.gu * u + k.gv * v) << 8) |
         ((unsigned)frmap_yuv_clip8(l + k.bu * u) << 16);
}

// What a frame record must satisfy before a sample of it is read: planes, chroma step, table row, pitches.
FRMAP_YUV_HD inline bool frmap_yuv_frame_ok(const FrmapYuvFrame& f) {
  if (!f.y || !f.u || !f.v || f.H < 1 || f.W < 1) return false;
  if (f.c_step != 1 && f.c_step != 2) return false;
  if (f.csc < 0 || f.csc >= FRMAP_YUV_CSC_COUNT) return false;
  return f.y_pitch >= (long long)f.W && f.c_pitch >= (long long)f.c_step * (((long long)f.W + 1) >> 1);
}

// Pixel (x, y) of the frame, 0 <= x < W, 0 <= y < H, as R | G << 8 | B << 16 (k = frmap_yuv_csc(f.csc)).  Plane offsets in 64 bits.
FRMAP_YUV_HD inline unsigned frmap_yuv_pixel(const FrmapYuvFrame& f, const FrmapYuvCsc& k, int x, int y) {
  const long long yo = (long long)y * f.y_pitch + (long long)x;
  const long long co = (long long)(y >> 1) * f.c_pitch + (long long)(x >> 1) * (long long)f.c_step;
  return frmap_yuv_rgb(((const unsigned char*)f.y)[yo], ((const unsigned char*)f.u)[co], ((const unsigned char*)f.v)[co], k);
}
FRMAP_YUV_HD inline unsigned frmap_yuv_pixel(const FrmapYuvFrame& f, int x, int y) {
  return frmap_yuv_pixel(f, frmap_yuv_csc(f.csc), x, y);
}

// The YUV form of frmap_align_warp_pixel (align_crop.hip): pixel (x, y) of Image.rotate's output for the CONVERTED frame and the
// output -> input matrix m[6].  The four corner pixels of the bilinear warp are converted to uint8 RGB first; Pillow's float64
// arithmetic (affine_transform + bilinear_filter32RGB, nothing fused) then runs on those.  Every index is clamped to the frame and
// a sample outside it (NaN coordinates included) is RGB (0, 0, 0), so nothing is read outside the planes whatever the matrix holds.
FRMAP_YUV_HD inline unsigned frmap_yuv_warp_pixel(const FrmapYuvFrame& f, const FrmapYuvCsc& k, const double* m, int x, int y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int H = f.H, W = f.W;
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
  const unsigned p00 = frmap_yuv_pixel(f, k, xa, ya), p01 = frmap_yuv_pixel(f, k, xb, ya);
  unsigned p10 = 0u, p11 = 0u;
  if (below) {
    p10 = frmap_yuv_pixel(f, k, xa, yi + 1);
    p11 = frmap_yuv_pixel(f, k, xb, yi + 1);
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

// ---- the host twins: HOST pointers in the record.  nullptr = done; otherwise the reason the call is refused, nothing written.
inline const char* frmap_yuv_host_frame(FrmapYuvFrame* f, const unsigned char* y, const unsigned char* u, const unsigned char* v, int H,
                                        int W, long long y_pitch, long long c_pitch, int c_step, int csc) {
  if (!y || !u || !v) return "null pointer";
  if (H < 1 || W < 1) return "frame size is not positive";
  if (c_step != 1 && c_step != 2) return "c_step is neither 1 nor 2";
  if (csc < 0 || csc >= FRMAP_YUV_CSC_COUNT) return "csc lies outside [0, 4)";
  if (y_pitch < (long long)W) return "y_pitch is below the frame's width";
  if (c_pitch < (long long)c_step * (((long long)W + 1) >> 1)) return "c_pitch is below c_step * ceil(W / 2)";
  f->y = (unsigned long long)(size_t)y;
  f->u = (unsigned long long)(size_t)u;
  f->v = (unsigned long long)(size_t)v;
  f->H = H;
  f->W = W;
  f->y_pitch = y_pitch;
  f->c_pitch = c_pitch;
  f->c_step = c_step;
  f->csc = csc;
  return nullptr;
}

inline void frmap_yuv_store3(unsigned char* o, unsigned v) {
  o[0] = (unsigned char)(v & 255u);
  o[1] = (unsigned char)((v >> 8) & 255u);
  o[2] = (unsigned char)((v >> 16) & 255u);
}

// the whole frame converted: out_rgb [H][W][3], packed
inline const char* frmap_yuv_to_rgb_twin(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W,
                                         long long y_pitch, long long c_pitch, int c_step, int csc, unsigned char* out_rgb) {
  FrmapYuvFrame f;
  if (!out_rgb) return "null pointer";
  if (const char* why = frmap_yuv_host_frame(&f, y, u, v, H, W, y_pitch, c_pitch, c_step, csc)) return why;
  const FrmapYuvCsc k = frmap_yuv_csc(csc);
  for (int yy = 0; yy < H; ++yy)
    for (int xx = 0; xx < W; ++xx) frmap_yuv_store3(out_rgb + ((size_t)yy * (size_t)W + (size_t)xx) * 3, frmap_yuv_pixel(f, k, xx, yy));
  return nullptr;
}

// rows [y1, y2), columns [x1, x2) of Image.rotate's output for the converted frame: out [y2 - y1][x2 - x1][3]
inline const char* frmap_yuv_align_warp_twin(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W,
                                             long long y_pitch, long long c_pitch, int c_step, int csc, const double* mat6, int x1, int y1,
                                             int x2, int y2, unsigned char* out) {
  FrmapYuvFrame f;
  if (!mat6 || !out) return "null pointer";
  if (const char* why = frmap_yuv_host_frame(&f, y, u, v, H, W, y_pitch, c_pitch, c_step, csc)) return why;
  if (!(x1 >= 0 && y1 >= 0 && x2 <= W && y2 <= H && x2 > x1 && y2 > y1)) return "ROI is empty or leaves its frame";
  for (int i = 0; i < 6; ++i)
    if (!isfinite(mat6[i])) return "a matrix entry is not finite";
  const FrmapYuvCsc k = frmap_yuv_csc(csc);
  for (int yy = y1; yy < y2; ++yy)
    for (int xx = x1; xx < x2; ++xx)
      frmap_yuv_store3(out + ((size_t)(yy - y1) * (size_t)(x2 - x1) + (size_t)(xx - x1)) * 3, frmap_yuv_warp_pixel(f, k, mat6, xx, yy));
  return nullptr;
}
