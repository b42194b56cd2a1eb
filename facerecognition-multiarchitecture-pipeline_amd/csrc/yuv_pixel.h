// One pixel of a 4:2:0 YUV frame as RGB, for the host and the device alike: the YUV sources of the crop body (yuv_crop.hip,
// crop_device.h) convert a filter tap's pixel where the tap reads it, so no RGB frame is ever written; frmap_yuv_to_rgb_host /
// frmap_yuv_align_warp_host run the same text on the CPU (the warp itself is rgb_pixel.h's) and tools/yuv_check.cpp includes it
// under a plain C++ compiler with the sanitizers.  Not part of the public ABI.
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
#include "frame_records.h"
#include "rgb_pixel.h"

constexpr int FRMAP_YUV_CSC_COUNT = 4;

struct FrmapYuvCsc {
  int y_off, cy, rv, gu, gv, bu;
};

// row `csc` of the table (frames.YUV_COEFFS); csc outside [0, 4) is the caller's to refuse
FRMAP_HD inline FrmapYuvCsc frmap_yuv_csc(int csc) {
  switch (csc) {
    case 0: return FrmapYuvCsc{16, 76309, 104597, -25675, -53279, 132201};    // bt601, limited
    case 1: return FrmapYuvCsc{0, 65536, 91881, -22553, -46802, 116130};      // bt601, full
    case 2: return FrmapYuvCsc{16, 76309, 117489, -13975, -34925, 138438};    // bt709, limited
    default: return FrmapYuvCsc{0, 65536, 103206, -12276, -30679, 121609};    // bt709, full
  }
}

FRMAP_HD inline int frmap_yuv_clip8(int v) {
  v >>= 16;                                                                   // arithmetic: v may be negative
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (Y, U, V) -> R | G << 8 | B << 16
FRMAP_HD inline unsigned frmap_yuv_rgb(int Y, int U, int V, const FrmapYuvCsc& k) {
  const int l = k.cy * (Y - k.y_off) + 32768, u = U - 128, v = V - 128;
  return (unsigned)frmap_yuv_clip8(l + k.rv * v) | ((unsigned)frmap_yuv_clip8(l + k.gu * u + k.gv * v) << 8) |
         ((unsigned)frmap_yuv_clip8(l + k.bu * u) << 16);
}

// What a frame record must satisfy before a sample of it is read: planes, chroma step, table row, pitches.
FRMAP_HD inline bool frmap_yuv_frame_ok(const FrmapYuvFrame& f) {
  if (!f.y || !f.u || !f.v || f.H < 1 || f.W < 1) return false;
  if (f.c_step != 1 && f.c_step != 2) return false;
  if (f.csc < 0 || f.csc >= FRMAP_YUV_CSC_COUNT) return false;
  return f.y_pitch >= (long long)f.W && f.c_pitch >= (long long)f.c_step * (((long long)f.W + 1) >> 1);
}

// Pixel (x, y) of the frame, 0 <= x < W, 0 <= y < H, as R | G << 8 | B << 16 (k = frmap_yuv_csc(f.csc)).  Plane offsets in 64 bits.
FRMAP_HD inline unsigned frmap_yuv_pixel(const FrmapYuvFrame& f, const FrmapYuvCsc& k, int x, int y) {
  const long long yo = (long long)y * f.y_pitch + (long long)x;
  const long long co = (long long)(y >> 1) * f.c_pitch + (long long)(x >> 1) * (long long)f.c_step;
  return frmap_yuv_rgb(((const unsigned char*)f.y)[yo], ((const unsigned char*)f.u)[co], ((const unsigned char*)f.v)[co], k);
}
FRMAP_HD inline unsigned frmap_yuv_pixel(const FrmapYuvFrame& f, int x, int y) {
  return frmap_yuv_pixel(f, frmap_yuv_csc(f.csc), x, y);
}

// What frmap_warp_pixel (rgb_pixel.h) fetches for the aligned crop of a YUV frame: the four corner pixels of the bilinear warp are
// converted to uint8 RGB first, Pillow's float64 arithmetic then runs on those, and what rotates in from outside is RGB (0, 0, 0).
struct FrmapYuvFetch {
  FrmapYuvFrame f;
  FrmapYuvCsc k;
  FRMAP_HD unsigned operator()(int x, int y) const { return frmap_yuv_pixel(f, k, x, y); }
};

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

// the whole frame converted: out_rgb [H][W][3], packed
inline const char* frmap_yuv_to_rgb_twin(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W,
                                         long long y_pitch, long long c_pitch, int c_step, int csc, unsigned char* out_rgb) {
  FrmapYuvFrame f;
  if (!out_rgb) return "null pointer";
  if (const char* why = frmap_yuv_host_frame(&f, y, u, v, H, W, y_pitch, c_pitch, c_step, csc)) return why;
  const FrmapYuvCsc k = frmap_yuv_csc(csc);
  for (int yy = 0; yy < H; ++yy)
    for (int xx = 0; xx < W; ++xx) frmap_rgb_store3(out_rgb + ((size_t)yy * (size_t)W + (size_t)xx) * 3, frmap_yuv_pixel(f, k, xx, yy));
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
  const FrmapYuvFetch fetch{f, frmap_yuv_csc(csc)};
  for (int yy = y1; yy < y2; ++yy)
    for (int xx = x1; xx < x2; ++xx)
      frmap_rgb_store3(out + ((size_t)(yy - y1) * (size_t)(x2 - x1) + (size_t)(xx - x1)) * 3, frmap_warp_pixel(H, W, mat6, xx, yy, fetch));
  return nullptr;
}
