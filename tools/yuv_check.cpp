// The pixel functions of the crop kernels (csrc/yuv_pixel.h: the conversion; csrc/rgb_pixel.h: the warp pixel every source shares
// and the read of a packed frame - the text the kernels compile) under the address and undefined-behaviour sanitizers, as a
// stand-alone host program: no Python, no GPU; host-only work, not for a machine with a GPU.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Ifacerecognition-multiarchitecture-pipeline_amd/csrc tools/yuv_check.cpp -o /tmp/yuv_check && /tmp/yuv_check
//
// Every plane lives in a heap buffer of EXACTLY the size the record states ((rows - 1) * pitch + the bytes of the last row), so a
// read one sample outside is a sanitizer report.  Frames: 1 x 1, 2 x 2, 5 x 7, 37 x 53 and 6 x 8, planar (c_step 1) and
// interleaved (c_step 2, u first and v first), tight and padded pitches, all four csc rows, random bytes (every clip branch).
// The conversion is compared with the formula written out a second time here; the warp with the identity matrix must be the
// conversion, with matrices that throw every sample outside the frame it must be zero, and with tilted ones (samples on every
// clamped edge and outside) it must equal Pillow's bilinear arithmetic applied to the converted frame.  Bad arguments must be
// refused with the output untouched.  The packed source: the same warp, matrices and ROIs over the converted picture held as a
// packed RGB and a packed BGR buffer of exactly the stated size, tight and padded pitch, against the same reference.  Prints
// "yuv_check passed" and returns 0, or says what differed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "yuv_pixel.h"

static uint32_t g_seed = 20251019u;
static unsigned char next_byte() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (unsigned char)(g_seed >> 24);
}

static const int TABLE[4][6] = {{16, 76309, 104597, -25675, -53279, 132201}, {0, 65536, 91881, -22553, -46802, 116130},
                                {16, 76309, 117489, -13975, -34925, 138438}, {0, 65536, 103206, -12276, -30679, 121609}};

static int clip8(long long v) {
  const long long s = v >= 0 ? v / 65536 : -((-v + 65535) / 65536);          // floor division: the arithmetic shift, written out
  return s < 0 ? 0 : (s > 255 ? 255 : (int)s);
}

struct Frame {
  int H, W, c_step, csc;
  long long y_pitch, c_pitch;
  bool v_first;
  std::vector<unsigned char> y, c0, c1;                                    // interleaved: c0 holds both, c1 is empty
  const unsigned char* u() const { return c_step == 2 ? c0.data() + (v_first ? 1 : 0) : c0.data(); }
  const unsigned char* v() const { return c_step == 2 ? c0.data() + (v_first ? 0 : 1) : c1.data(); }
};

static Frame make_frame(int H, int W, int c_step, bool v_first, int csc, int y_pad, int c_pad) {
  Frame f;
  f.H = H; f.W = W; f.c_step = c_step; f.csc = csc; f.v_first = v_first;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;
  f.y_pitch = W + y_pad;
  f.c_pitch = (long long)c_step * cw + c_pad;
  f.y.resize((size_t)((H - 1) * f.y_pitch + W));
  f.c0.resize((size_t)((ch - 1) * f.c_pitch + (long long)c_step * cw));
  if (c_step == 1) f.c1.resize(f.c0.size());
  for (auto& b : f.y) b = next_byte();
  for (auto& b : f.c0) b = next_byte();
  for (auto& b : f.c1) b = next_byte();
  return f;
}

static void reference_rgb(const Frame& f, std::vector<unsigned char>& out) {
  const int* k = TABLE[f.csc];
  out.assign((size_t)f.H * f.W * 3, 0);
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x) {
      const long long Y = f.y[(size_t)(y * f.y_pitch + x)] - k[0];
      const size_t co = (size_t)((y / 2) * f.c_pitch + (long long)(x / 2) * f.c_step);
      const long long U = f.u()[co] - 128, V = f.v()[co] - 128;
      unsigned char* o = &out[((size_t)y * f.W + x) * 3];
      o[0] = (unsigned char)clip8(k[1] * Y + k[2] * V + 32768);
      o[1] = (unsigned char)clip8(k[1] * Y + k[3] * U + k[4] * V + 32768);
      o[2] = (unsigned char)clip8(k[1] * Y + k[5] * U + 32768);
    }
}

// Pillow's affine transform with the bilinear filter on the converted frame (rgb_pixel.h's arithmetic), written a second time on the RGB array
static void reference_warp(const std::vector<unsigned char>& rgb, int H, int W, const double* m, int x, int y, unsigned char* o) {
  o[0] = o[1] = o[2] = 0;
  const double xo = x + 0.5, yo = y + 0.5;
  double xin = m[0] * xo + m[1] * yo + m[2], yin = m[3] * xo + m[4] * yo + m[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return;
  xin -= 0.5;
  yin -= 0.5;
  const int xi = (int)floor(xin), yi = (int)floor(yin);
  const double dx = xin - xi, dy = yin - yi;
  const int xa = xi < 0 ? 0 : xi, xb = xi + 1 < W ? xi + 1 : W - 1, ya = yi < 0 ? 0 : yi;
  for (int c = 0; c < 3; ++c) {
    const int a0 = rgb[((size_t)ya * W + xa) * 3 + c], a1 = rgb[((size_t)ya * W + xb) * 3 + c];
    const double v1 = a0 + (a1 - a0) * dx;
    double v2 = v1;
    if (yi + 1 < H) {
      const int b0 = rgb[((size_t)(yi + 1) * W + xa) * 3 + c], b1 = rgb[((size_t)(yi + 1) * W + xb) * 3 + c];
      v2 = b0 + (b1 - b0) * dx;
    }
    o[c] = (unsigned char)(int)(v1 + (v2 - v1) * dy);
  }
}

static int g_packed = 0;   // packed-source cases run: frame x matrix x ROI x (RGB | BGR) x (tight | padded)

static int fail(const char* what, const Frame& f) {
  printf("yuv_check: %s (frame %d x %d, c_step %d, v first %d, csc %d, pitches %lld / %lld)\n", what, f.H, f.W, f.c_step, (int)f.v_first,
         f.csc, f.y_pitch, f.c_pitch);
  return 1;
}

static int check_frame(const Frame& f) {
  std::vector<unsigned char> want, got((size_t)f.H * f.W * 3, 0xA5);
  reference_rgb(f, want);
  if (frmap_yuv_to_rgb_twin(f.y.data(), f.u(), f.v(), f.H, f.W, f.y_pitch, f.c_pitch, f.c_step, f.csc, got.data())) return fail("conversion refused", f);
  if (got != want) return fail("conversion differs from the formula", f);
  // the packed source's four buffers: the converted picture as RGB and as BGR, rows of a tight and of a padded `pitch`, each
  // buffer ending with the last pixel of its last row
  struct Packed { std::vector<unsigned char> bytes; long long pitch; int c0; };
  std::vector<Packed> packed;
  for (int variant = 0; variant < 4; ++variant) {
    Packed pk;
    pk.c0 = variant & 1 ? 2 : 0;
    pk.pitch = 3LL * f.W + (variant & 2 ? 7 : 0);
    pk.bytes.resize((size_t)((f.H - 1) * pk.pitch + 3LL * f.W));
    for (int y = 0; y < f.H; ++y)
      for (int x = 0; x < f.W; ++x)
        for (int c = 0; c < 3; ++c)
          pk.bytes[(size_t)(y * pk.pitch + 3LL * x + (c == 1 ? 1 : (c == 0 ? pk.c0 : 2 - pk.c0)))] = want[((size_t)y * f.W + x) * 3 + c];
    packed.push_back(pk);
  }
  const double cx = f.W / 2.0, cy = f.H / 2.0;
  const double mats[][6] = {
      {1.0, 0.0, 0.0, 0.0, 1.0, 0.0},                                          // identity: the conversion itself
      {1.0, 0.0, 1e6, 0.0, 1.0, 0.0},                                          // every sample outside, to the right
      {1.0, 0.0, 0.0, 0.0, 1.0, -1e6},                                         // above
      {-1.0, 0.0, -3.0, 0.0, -1.0, -3.0},                                      // half a turn about a point outside: all outside
      {0.8, -0.6, cx - 0.8 * cx + 0.6 * cy, 0.6, 0.8, cy - 0.6 * cx - 0.8 * cy},             // tilted about the centre: corners outside
      {0.0, -1.0, cx + cy, 1.0, 0.0, cy - cx},                                 // a quarter turn
      {1.0, 0.0, 0.25, 0.0, 1.0, -0.25},                                       // a quarter pixel: samples on the clamped edges
      {1.0, 0.0, -0.75, 0.0, 1.0, 0.75},
      {0.5, 0.0, 0.0, 0.0, 0.5, 0.0},
      {3.0, 0.1, -f.W * 1.0, -0.1, 3.0, -f.H * 1.0},                           // most samples outside on every side
  };
  const int rois[][4] = {{0, 0, f.W, f.H}, {f.W / 2, f.H / 2, f.W, f.H}, {f.W - 1, f.H - 1, f.W, f.H}};
  for (int mi = 0; mi < (int)(sizeof(mats) / sizeof(mats[0])); ++mi)
    for (const auto& r : rois) {
      const double* m = mats[mi];
      const int w = r[2] - r[0], h = r[3] - r[1];
      std::vector<unsigned char> out((size_t)w * h * 3, 0xA5);                 // exactly the stated size
      if (frmap_yuv_align_warp_twin(f.y.data(), f.u(), f.v(), f.H, f.W, f.y_pitch, f.c_pitch, f.c_step, f.csc, m, r[0], r[1], r[2], r[3], out.data()))
        return fail("warp refused", f);
      for (int y = r[1]; y < r[3]; ++y)
        for (int x = r[0]; x < r[2]; ++x) {
          unsigned char o[3];
          reference_warp(want, f.H, f.W, m, x, y, o);
          if (memcmp(o, &out[((size_t)(y - r[1]) * w + (x - r[0])) * 3], 3) != 0) return fail("warp differs from the warp of the converted frame", f);
        }
      if (mi <= 3)                                                           // stated directly, not through the reference warp
        for (int y = r[1]; y < r[3]; ++y)
          for (int x = r[0]; x < r[2]; ++x)
            for (int c = 0; c < 3; ++c) {
              const unsigned char w0 = mi == 0 ? want[((size_t)y * f.W + x) * 3 + c] : 0;
              if (out[((size_t)(y - r[1]) * w + (x - r[0])) * 3 + c] != w0) return fail("identity / all-outside warp is not the conversion / zero", f);
            }
      for (const Packed& pk : packed)                                          // the packed source, against the same reference
        for (int y = r[1]; y < r[3]; ++y)
          for (int x = r[0]; x < r[2]; ++x) {
            unsigned char o[3], g[3];
            reference_warp(want, f.H, f.W, m, x, y, o);
            frmap_rgb_store3(g, frmap_warp_pixel(f.H, f.W, m, x, y, FrmapPackedFetch{pk.bytes.data(), pk.pitch, pk.c0}));
            if (memcmp(o, g, 3) != 0) return fail("packed warp differs from the warp of the converted frame", f);
          }
      g_packed += 4;
    }
  return 0;
}

static int check_rejections() {
  const Frame f = make_frame(5, 7, 2, false, 0, 0, 0);
  std::vector<unsigned char> out((size_t)5 * 7 * 3, 0xA5), before;
  before = out;
  const double eye[6] = {1, 0, 0, 0, 1, 0};
  double nan6[6] = {1, 0, 0, 0, 1, 0};
  nan6[4] = NAN;
  const unsigned char *y = f.y.data(), *u = f.u(), *v = f.v();
  int refused = 0, tried = 0;
#define REFUSED(call) do { ++tried; if ((call) != nullptr) ++refused; } while (0)
  REFUSED(frmap_yuv_to_rgb_twin(nullptr, u, v, 5, 7, 7, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, nullptr, v, 5, 7, 7, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, nullptr, 5, 7, 7, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 8, 2, 0, nullptr));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 0, 7, 7, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, -1, 7, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 8, 3, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 8, 0, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 8, 2, 4, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 8, 2, -1, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 6, 8, 2, 0, out.data()));
  REFUSED(frmap_yuv_to_rgb_twin(y, u, v, 5, 7, 7, 7, 2, 0, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, nullptr, 0, 0, 7, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, eye, 0, 0, 7, 5, nullptr));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, nan6, 0, 0, 7, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, eye, 0, 0, 8, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, eye, 0, 0, 7, 6, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, eye, -1, 0, 7, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 0, eye, 3, 2, 3, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 3, 0, eye, 0, 0, 7, 5, out.data()));
  REFUSED(frmap_yuv_align_warp_twin(y, u, v, 5, 7, 7, 8, 2, 4, eye, 0, 0, 7, 5, out.data()));
#undef REFUSED
  if (refused != tried) { printf("yuv_check: %d of %d bad calls were refused\n", refused, tried); return 1; }
  if (out != before) { printf("yuv_check: a refused call wrote its output\n"); return 1; }
  return 0;
}

int main() {
  const int sizes[][2] = {{1, 1}, {2, 2}, {5, 7}, {37, 53}, {6, 8}, {1, 9}, {9, 1}};
  int frames = 0;
  for (const auto& hw : sizes)
    for (int layout = 0; layout < 3; ++layout)                                 // planar, interleaved u first, interleaved v first
      for (int csc = 0; csc < 4; ++csc)
        for (int pad = 0; pad < 2; ++pad) {
          const Frame f = make_frame(hw[0], hw[1], layout == 0 ? 1 : 2, layout == 2, csc, pad ? 13 : 0, pad ? 6 : 0);
          if (check_frame(f)) return 1;
          ++frames;
        }
  if (check_rejections()) return 1;
  printf("yuv_check passed: %d frames, %d packed warp cases\n", frames, g_packed);
  return 0;
}
