// Face crops straight from 4:2:0 YUV frames (NV12 / NV21 surfaces of a hardware decoder, planar I420 / YV12 of a software one):
// YUV -> RGB + ROI crop + (optionally) the eye-alignment rotation + Pillow-exact bilinear resize in one launch, no RGB frame in
// memory.  Crop i equals, bit for bit, frmap_crop_resize_u8 / frmap_align_crop_resize_u8 on the frame converted by the rule of
// yuv_pixel.h (nearest chroma, 16-bit fixed-point colour; DESIGN.md section 4, "YUV frames").
//
// The kernels are crop_resize.hip's and align_crop.hip's - tap tables from resize_coeffs.h in LDS, the horizontal pass rounded to
// 8 bits in LDS, the vertical pass out of LDS, an axis whose size is unchanged copied, the launch shape of frmap_crop_plan - with
// one difference: a tap's source pixel is not a byte triple of a packed frame but frmap_yuv_pixel (three samples, converted and
// clipped to uint8 BEFORE they enter the resize sum) or, aligned, frmap_yuv_warp_pixel (the four corners converted first, then
// Pillow's float64 warp).  Both kernels are one body, templated on whether a matrix is applied.
#include "frame_records.h"
#include "frmap_common.h"
#include "resize_coeffs.h"
#include "yuv_pixel.h"

static_assert(sizeof(FrmapYuvFrame) == 56, "FrmapYuvFrame is mirrored by resize.py and described in frmap_hip.h as 56 bytes");

__device__ __forceinline__ int yuv_crop_clip8(int v) {
  v >>= FRMAP_RESIZE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <bool ALIGN>
__device__ __forceinline__ void yuv_crop_body(const FrmapYuvFrame* __restrict__ frames, int n_frames, const FrmapRoi* __restrict__ rois,
                                              const double* __restrict__ mats, unsigned char* __restrict__ out, int out_h, int out_w,
                                              int rows_per_block, int groups, int lds_rows, int ksx_cap, int ksy_cap) {
  extern __shared__ int s_mem[];
  unsigned* s_tmp = (unsigned*)s_mem;                 // [lds_rows][out_w] packed R | G << 8 | B << 16
  int* kx = s_mem + lds_rows * out_w;                 // [out_w][ksx_cap]
  int* bx = kx + out_w * ksx_cap;                     // [out_w][2] = (first input column, taps)
  int* ky = bx + 2 * out_w;                           // [rows_per_block][ksy_cap]
  int* by = ky + rows_per_block * ksy_cap;            // [rows_per_block][2]
  const int item = blockIdx.x / groups, grp = blockIdx.x - item * groups;
  const int y0 = grp * rows_per_block, y1 = min(y0 + rows_per_block, out_h), ny = y1 - y0;
  const FrmapRoi r = rois[item];
  // The frame, ROI and matrix records are device data the host call never saw.  A record that breaks the contract, or is larger
  // than the launch was sized for, is not processed (its output stays unwritten): nothing is read outside a plane or written
  // outside LDS.  Every test below is uniform over the workgroup, so all of its threads leave together.
  if ((unsigned)r.frame >= (unsigned)n_frames) return;
  const FrmapYuvFrame f = frames[r.frame];
  if (!frmap_yuv_frame_ok(f)) return;
  if (r.x1 < 0 || r.y1 < 0 || r.x2 > f.W || r.y2 > f.H || r.x2 <= r.x1 || r.y2 <= r.y1) return;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (ALIGN) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      m[i] = mats[(size_t)item * 6 + i];
      if (!__builtin_isfinite(m[i])) return;
    }
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
  const FrmapYuvCsc k3 = frmap_yuv_csc(f.csc);
  // ---- horizontal pass (ImagingResampleHorizontal_8bpc) over the needed rows of the converted (and rotated) image
  for (int idx = threadIdx.x; idx < nrows * out_w; idx += 256) {
    const int rr = idx / out_w, xx = idx - rr * out_w;
    const int y = r.y1 + row_first + rr;
    unsigned v;
    if (rx) {
      const int xmin = bx[2 * xx], cnt = bx[2 * xx + 1];
      const int* k = kx + xx * ksx_cap;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int x = 0; x < cnt; ++x) {
        const unsigned t = ALIGN ? frmap_yuv_warp_pixel(f, k3, m, r.x1 + xmin + x, y) : frmap_yuv_pixel(f, k3, r.x1 + xmin + x, y);
        const int w = k[x];
        s0 += (int)(t & 255u) * w; s1 += (int)((t >> 8) & 255u) * w; s2 += (int)((t >> 16) & 255u) * w;
      }
      v = (unsigned)yuv_crop_clip8(s0) | ((unsigned)yuv_crop_clip8(s1) << 8) | ((unsigned)yuv_crop_clip8(s2) << 16);
    } else {
      v = ALIGN ? frmap_yuv_warp_pixel(f, k3, m, r.x1 + xx, y) : frmap_yuv_pixel(f, k3, r.x1 + xx, y);
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
      v = (unsigned)yuv_crop_clip8(s0) | ((unsigned)yuv_crop_clip8(s1) << 8) | ((unsigned)yuv_crop_clip8(s2) << 16);
    } else {
      v = s_tmp[j * out_w + xx];
    }
    unsigned char* o = dst + ((size_t)yy * out_w + xx) * 3;
    o[0] = (unsigned char)(v & 255u); o[1] = (unsigned char)((v >> 8) & 255u); o[2] = (unsigned char)((v >> 16) & 255u);
  }
}

__global__ __launch_bounds__(256) void crop_resize_yuv_kernel(const FrmapYuvFrame* __restrict__ frames, int n_frames,
                                                              const FrmapRoi* __restrict__ rois, unsigned char* __restrict__ out,
                                                              int out_h, int out_w, int rows_per_block, int groups, int lds_rows,
                                                              int ksx_cap, int ksy_cap) {
  yuv_crop_body<false>(frames, n_frames, rois, nullptr, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap, ksy_cap);
}

__global__ __launch_bounds__(256) void align_crop_resize_yuv_kernel(const FrmapYuvFrame* __restrict__ frames, int n_frames,
                                                                    const FrmapRoi* __restrict__ rois, const double* __restrict__ mats,
                                                                    unsigned char* __restrict__ out, int out_h, int out_w,
                                                                    int rows_per_block, int groups, int lds_rows, int ksx_cap,
                                                                    int ksy_cap) {
  yuv_crop_body<true>(frames, n_frames, rois, mats, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap, ksy_cap);
}

extern "C" int frmap_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h,
                                     int out_w, int max_roi_h, int max_roi_w, void* stream) {
  FRMAP_REQUIRE(N >= 0, "crop_resize_yuv: N = %d", N);
  if (N == 0) return 0;
  FRMAP_REQUIRE(frames && rois && out, "crop_resize_yuv: null pointer");
  FRMAP_REQUIRE(n_frames > 0 && out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536 && max_roi_h > 0 && max_roi_w > 0 &&
                    max_roi_h <= (1 << 24) && max_roi_w <= (1 << 24),
                "crop_resize_yuv: bad shape");
  const FrmapCropPlan p = frmap_crop_plan(out_h, out_w, max_roi_h, max_roi_w);
  FRMAP_REQUIRE(p.lds <= FRMAP_CROP_LDS_MAX, "crop_resize_yuv: ROIs of up to %d x %d to %d x %d need %lld bytes of LDS for one output row (limit %d)",
                max_roi_h, max_roi_w, out_h, out_w, p.lds, FRMAP_CROP_LDS_MAX);
  FRMAP_REQUIRE((long long)N * p.groups <= 0x7fffffffLL, "crop_resize_yuv: %d ROIs x %d row groups exceed the grid", N, p.groups);
  if (frmap_big_lds((const void*)crop_resize_yuv_kernel, FRMAP_CROP_LDS_MAX)) return -2;
  hipLaunchKernelGGL(crop_resize_yuv_kernel, dim3((unsigned)(N * p.groups)), dim3(256), (size_t)p.lds, (hipStream_t)stream,
                     (const FrmapYuvFrame*)frames, n_frames, (const FrmapRoi*)rois, out, out_h, out_w, p.rows_per_block, p.groups,
                     p.lds_rows, p.ksx, p.ksy);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_align_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out,
                                           int N, int out_h, int out_w, int max_roi_h, int max_roi_w, void* stream) {
  FRMAP_REQUIRE(N >= 0, "align_crop_resize_yuv: N = %d", N);
  if (N == 0) return 0;
  FRMAP_REQUIRE(frames && rois && mats && out, "align_crop_resize_yuv: null pointer");
  FRMAP_REQUIRE(((uintptr_t)mats & 7) == 0, "align_crop_resize_yuv: mats must be 8-byte aligned");
  FRMAP_REQUIRE(n_frames > 0 && out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536 && max_roi_h > 0 && max_roi_w > 0 &&
                    max_roi_h <= (1 << 24) && max_roi_w <= (1 << 24),
                "align_crop_resize_yuv: bad shape");
  const FrmapCropPlan p = frmap_crop_plan(out_h, out_w, max_roi_h, max_roi_w);
  FRMAP_REQUIRE(p.lds <= FRMAP_CROP_LDS_MAX,
                "align_crop_resize_yuv: ROIs of up to %d x %d to %d x %d need %lld bytes of LDS for one output row (limit %d)", max_roi_h,
                max_roi_w, out_h, out_w, p.lds, FRMAP_CROP_LDS_MAX);
  FRMAP_REQUIRE((long long)N * p.groups <= 0x7fffffffLL, "align_crop_resize_yuv: %d ROIs x %d row groups exceed the grid", N, p.groups);
  if (frmap_big_lds((const void*)align_crop_resize_yuv_kernel, FRMAP_CROP_LDS_MAX)) return -2;
  hipLaunchKernelGGL(align_crop_resize_yuv_kernel, dim3((unsigned)(N * p.groups)), dim3(256), (size_t)p.lds, (hipStream_t)stream,
                     (const FrmapYuvFrame*)frames, n_frames, (const FrmapRoi*)rois, mats, out, out_h, out_w, p.rows_per_block, p.groups,
                     p.lds_rows, p.ksx, p.ksy);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_yuv_to_rgb_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W,
                                     long long y_pitch, long long c_pitch, int c_step, int csc, unsigned char* out_rgb) {
  const char* why = frmap_yuv_to_rgb_twin(y, u, v, H, W, y_pitch, c_pitch, c_step, csc, out_rgb);
  FRMAP_REQUIRE(!why, "yuv_to_rgb_host: %s (frame %d x %d, y_pitch %lld, c_pitch %lld, c_step %d, csc %d)", why, H, W, y_pitch, c_pitch,
                c_step, csc);
  return 0;
}

extern "C" int frmap_yuv_align_warp_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W,
                                         long long y_pitch, long long c_pitch, int c_step, int csc, const double* mat6, int x1, int y1,
                                         int x2, int y2, unsigned char* out) {
  const char* why = frmap_yuv_align_warp_twin(y, u, v, H, W, y_pitch, c_pitch, c_step, csc, mat6, x1, y1, x2, y2, out);
  FRMAP_REQUIRE(!why, "yuv_align_warp_host: %s (frame %d x %d, ROI (%d, %d, %d, %d), c_step %d, csc %d)", why, H, W, x1, y1, x2, y2,
                c_step, csc);
  return 0;
}
