// Eye-aligned face crops straight from device-resident frames: rotate about the point between the eyes, crop the (margin) box,
// optional BGR -> RGB, Pillow-exact bilinear resize - one launch for every face of a detector, no rotated frame in memory.  The
// reference's dataset step (src/data_prep.py:69-87, 144-150) rotates the whole image, crops and resizes, with cv2.warpAffine and
// cv2.resize.  DEPARTURE: the geometry is the reference's (angle, centre, "rotate the frame, then crop"), the RESAMPLING is
// Pillow's, which is what this project pins its image arithmetic to (resize.hip, crop_resize.hip): crop i equals, bit for bit,
//     Image.fromarray(rgb_frame).rotate(angle_i, resample=Image.BILINEAR, center=center_i)      (same size, fill 0)
//          .crop((x1, y1, x2, y2)).resize((out_w, out_h), Image.BILINEAR)
// and not what cv2 would give (another interpolation grid and fixed-point weights).
//
// The kernel is crop_resize.hip's - tap tables from resize_coeffs.h in LDS, the horizontal pass rounded to 8 bits in LDS, the
// vertical pass out of LDS, an axis whose size is unchanged copied - with one difference: a tap's source pixel is not a byte
// triple of the frame but the ROTATED image's pixel at that position, computed on the spot by frmap_align_warp_pixel (Pillow's
// Geometry.c: affine_transform + bilinear_filter32RGB, float64, from four pixels of the frame) and truncated to 8 bits BEFORE it
// enters the resize sum, because Pillow resizes the uint8 image that rotate() returned.  A warped pixel is recomputed by every
// tap that reads it (about two per pixel, whatever the scale) instead of being staged in LDS: the LDS need, and with it the
// launch shape and the supported reductions, stay exactly crop_resize.hip's; see DESIGN.md section 4, "Aligned crops".
//
// The host computes each face's output -> input matrix (Pillow rounds cos / sin to 15 DECIMALS, which only decimal arithmetic
// reproduces: frames.rotation_matrix); everything per pixel happens here.  As in resize_coeffs.h the float64 operation order is
// Pillow's and nothing may be fused into an FMA, so the warp turns contraction off.
#include "frame_records.h"
#include "frmap_common.h"
#include "resize_coeffs.h"

// Pixel (x, y) of Image.rotate's output for the frame at `base` (H x W, 3 bytes per pixel, `pitch` bytes per row) and the
// output -> input matrix m[6], as R | G << 8 | B << 16 (c0 = the byte of a source pixel that holds R: 0, or 2 for BGR frames).
// Every index is clamped to the frame and a sample outside it (NaN coordinates included: the test is written so that NaN fails
// it) is 0, so nothing is read outside the frame whatever the matrix holds.
__host__ __device__ inline unsigned frmap_align_warp_pixel(const unsigned char* base, int H, int W, long long pitch, const double* m,
                                                           int x, int y, int c0) {
#pragma clang fp contract(off)
  const double xo = x + 0.5, yo = y + 0.5;
  double xin = m[0] * xo + m[1] * yo + m[2];
  double yin = m[3] * xo + m[4] * yo + m[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return 0u;
  xin -= 0.5;
  yin -= 0.5;
  const int xi = (int)floor(xin), yi = (int)floor(yin);          // in [-1, W - 1] x [-1, H - 1]
  const double dx = xin - xi, dy = yin - yi;
  const int xa = xi < 0 ? 0 : xi, xb = xi + 1 < W ? xi + 1 : W - 1, ya = yi < 0 ? 0 : yi;
  const unsigned char* r0 = base + (size_t)ya * pitch;
  const bool below = yi + 1 < H;                                 // (yi + 1 >= 0 always)
  const unsigned char* r1 = base + (size_t)(below ? yi + 1 : ya) * pitch;
  const unsigned char *p00 = r0 + 3 * xa, *p01 = r0 + 3 * xb, *p10 = r1 + 3 * xa, *p11 = r1 + 3 * xb;
  unsigned out = 0u;
  for (int c = 0; c < 3; ++c) {
    const int b = c == 1 ? 1 : (c == 0 ? c0 : 2 - c0);
    const int a0 = p00[b], a1 = p01[b];
    const double v1 = a0 + (a1 - a0) * dx;
    double v2 = v1;
    if (below) {
      const int b0 = p10[b], b1 = p11[b];
      v2 = b0 + (b1 - b0) * dx;
    }
    out |= (unsigned)(int)(v1 + (v2 - v1) * dy) << (8 * c);       // (UINT8) of a value in [0, 255]: truncation
  }
  return out;
}

__device__ __forceinline__ int align_clip8(int v) {
  v >>= FRMAP_RESIZE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void align_crop_resize_u8_kernel(const FrmapFrame* __restrict__ frames, int n_frames,
                                                                   const FrmapRoi* __restrict__ rois, const double* __restrict__ mats,
                                                                   unsigned char* __restrict__ out, int out_h, int out_w,
                                                                   int rows_per_block, int groups, int lds_rows, int ksx_cap,
                                                                   int ksy_cap, int bgr) {
  extern __shared__ int s_mem[];
  unsigned* s_tmp = (unsigned*)s_mem;                 // [lds_rows][out_w] packed R | G << 8 | B << 16
  int* kx = s_mem + lds_rows * out_w;                 // [out_w][ksx_cap]
  int* bx = kx + out_w * ksx_cap;                     // [out_w][2] = (first input column, taps)
  int* ky = bx + 2 * out_w;                           // [rows_per_block][ksy_cap]
  int* by = ky + rows_per_block * ksy_cap;            // [rows_per_block][2]
  const int item = blockIdx.x / groups, grp = blockIdx.x - item * groups;
  const int y0 = grp * rows_per_block, y1 = min(y0 + rows_per_block, out_h), ny = y1 - y0;
  const FrmapRoi r = rois[item];
  // The ROI and matrix records are device data the host call never saw.  A record that breaks the contract, or is larger than
  // the launch was sized for, is not processed (its output stays unwritten): nothing is read outside a frame or written outside
  // LDS.  The ROI lies in the rotated frame, which has the frame's size.
  if ((unsigned)r.frame >= (unsigned)n_frames) return;
  const FrmapFrame f = frames[r.frame];
  if (r.x1 < 0 || r.y1 < 0 || r.x2 > f.W || r.y2 > f.H || r.x2 <= r.x1 || r.y2 <= r.y1) return;
  double m[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    m[i] = mats[(size_t)item * 6 + i];
    if (!__builtin_isfinite(m[i])) return;
  }
  const int W = r.x2 - r.x1, H = r.y2 - r.y1;
  const bool rx = W != out_w, ry = H != out_h;
  const FrmapResizeAxis ax = frmap_resize_axis(W, out_w), ay = frmap_resize_axis(H, out_h);
  if ((rx && ax.ksize > ksx_cap) || (ry && ay.ksize > ksy_cap)) return;
  // ---- tap tables: one thread per output column, then per output row of this block
  for (int i = threadIdx.x; i < out_w + ny; i += 256) {
    if (i < out_w) {
      if (rx) frmap_resize_taps(ax, i, &bx[2 * i], &bx[2 * i + 1], kx + i * ksx_cap);
    } else if (ry) {
      const int j = i - out_w;
      frmap_resize_taps(ay, y0 + j, &by[2 * j], &by[2 * j + 1], ky + j * ksy_cap);
    }
  }
  __syncthreads();
  int row_first = y0, row_last = y1;                  // rows (of the ROI) this block's output rows read
  if (ry) {
    row_first = by[0];
    row_last = by[2 * (ny - 1)] + by[2 * (ny - 1) + 1];
  }
  const int nrows = row_last - row_first;
  if (nrows > lds_rows) return;
  const unsigned char* base = (const unsigned char*)f.base;
  const int c0 = bgr ? 2 : 0;                         // byte of a source pixel that holds R
  // ---- horizontal pass (ImagingResampleHorizontal_8bpc) over the needed rows of the rotated image
  for (int idx = threadIdx.x; idx < nrows * out_w; idx += 256) {
    const int rr = idx / out_w, xx = idx - rr * out_w;
    const int y = r.y1 + row_first + rr;
    unsigned v;
    if (rx) {
      const int xmin = bx[2 * xx], cnt = bx[2 * xx + 1];
      const int* k = kx + xx * ksx_cap;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int x = 0; x < cnt; ++x) {
        const unsigned t = frmap_align_warp_pixel(base, f.H, f.W, f.pitch, m, r.x1 + xmin + x, y, c0);
        const int w = k[x];
        s0 += (int)(t & 255u) * w; s1 += (int)((t >> 8) & 255u) * w; s2 += (int)((t >> 16) & 255u) * w;
      }
      v = (unsigned)align_clip8(s0) | ((unsigned)align_clip8(s1) << 8) | ((unsigned)align_clip8(s2) << 16);
    } else {
      v = frmap_align_warp_pixel(base, f.H, f.W, f.pitch, m, r.x1 + xx, y, c0);
    }
    s_tmp[idx] = v;
  }
  __syncthreads();
  // ---- vertical pass (ImagingResampleVertical_8bpc) out of LDS
  unsigned char* dst = out + ((size_t)item * out_h) * out_w * 3;
  for (int idx = threadIdx.x; idx < ny * out_w; idx += 256) {
    const int j = idx / out_w, xx = idx - j * out_w, yy = y0 + j;
    unsigned v;
    if (ry) {
      const int ymin = by[2 * j] - row_first, cnt = by[2 * j + 1];
      const int* k = ky + j * ksy_cap;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int y = 0; y < cnt; ++y) {
        const unsigned t = s_tmp[(ymin + y) * out_w + xx];
        const int w = k[y];
        s0 += (int)(t & 255u) * w; s1 += (int)((t >> 8) & 255u) * w; s2 += (int)((t >> 16) & 255u) * w;
      }
      v = (unsigned)align_clip8(s0) | ((unsigned)align_clip8(s1) << 8) | ((unsigned)align_clip8(s2) << 16);
    } else {
      v = s_tmp[j * out_w + xx];
    }
    unsigned char* o = dst + ((size_t)yy * out_w + xx) * 3;
    o[0] = (unsigned char)(v & 255u); o[1] = (unsigned char)((v >> 8) & 255u); o[2] = (unsigned char)((v >> 16) & 255u);
  }
}

extern "C" int frmap_align_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out,
                                          int N, int out_h, int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream) {
  FRMAP_REQUIRE(N >= 0, "align_crop_resize_u8: N = %d", N);
  if (N == 0) return 0;
  FRMAP_REQUIRE(frames && rois && mats && out, "align_crop_resize_u8: null pointer");
  FRMAP_REQUIRE(((uintptr_t)mats & 7) == 0, "align_crop_resize_u8: mats must be 8-byte aligned");
  FRMAP_REQUIRE(n_frames > 0 && out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536 && max_roi_h > 0 && max_roi_w > 0 &&
                    max_roi_h <= (1 << 24) && max_roi_w <= (1 << 24),
                "align_crop_resize_u8: bad shape");
  const FrmapCropPlan p = frmap_crop_plan(out_h, out_w, max_roi_h, max_roi_w);
  FRMAP_REQUIRE(p.lds <= FRMAP_CROP_LDS_MAX,
                "align_crop_resize_u8: ROIs of up to %d x %d to %d x %d need %lld bytes of LDS for one output row (limit %d)", max_roi_h,
                max_roi_w, out_h, out_w, p.lds, FRMAP_CROP_LDS_MAX);
  FRMAP_REQUIRE((long long)N * p.groups <= 0x7fffffffLL, "align_crop_resize_u8: %d ROIs x %d row groups exceed the grid", N, p.groups);
  if (frmap_big_lds((const void*)align_crop_resize_u8_kernel, FRMAP_CROP_LDS_MAX)) return -2;
  hipLaunchKernelGGL(align_crop_resize_u8_kernel, dim3((unsigned)(N * p.groups)), dim3(256), (size_t)p.lds, (hipStream_t)stream,
                     (const FrmapFrame*)frames, n_frames, (const FrmapRoi*)rois, mats, out, out_h, out_w, p.rows_per_block, p.groups,
                     p.lds_rows, p.ksx, p.ksy, bgr ? 1 : 0);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_align_warp_host(const unsigned char* frame, int H, int W, long long pitch, const double* mat6, int x1, int y1,
                                     int x2, int y2, int bgr, unsigned char* out) {
  FRMAP_REQUIRE(frame && mat6 && out, "align_warp_host: null pointer");
  FRMAP_REQUIRE(H > 0 && W > 0 && pitch >= 3LL * W, "align_warp_host: frame %d x %d, pitch %lld", H, W, pitch);
  FRMAP_REQUIRE(x1 >= 0 && y1 >= 0 && x2 <= W && y2 <= H && x2 > x1 && y2 > y1,
                "align_warp_host: ROI (%d, %d, %d, %d) is empty or leaves its %dx%d frame", x1, y1, x2, y2, W, H);
  for (int i = 0; i < 6; ++i) FRMAP_REQUIRE(isfinite(mat6[i]), "align_warp_host: matrix entry %d is not finite", i);
  for (int y = y1; y < y2; ++y)
    for (int x = x1; x < x2; ++x) {
      const unsigned v = frmap_align_warp_pixel(frame, H, W, pitch, mat6, x, y, bgr ? 2 : 0);
      unsigned char* o = out + ((size_t)(y - y1) * (x2 - x1) + (x - x1)) * 3;
      o[0] = (unsigned char)(v & 255u); o[1] = (unsigned char)((v >> 8) & 255u); o[2] = (unsigned char)((v >> 16) & 255u);
    }
  return 0;
}
