// Face crops straight from 4:2:0 YUV frames (NV12 / NV21 surfaces of a hardware decoder, planar I420 / YV12 of a software one):
// YUV -> RGB + ROI crop + (optionally) the eye-alignment rotation + Pillow-exact bilinear resize in one launch, no RGB frame in
// memory.  Crop i equals, bit for bit, frmap_crop_resize_u8 / frmap_align_crop_resize_u8 on the frame converted by the rule of
// yuv_pixel.h (nearest chroma, 16-bit fixed-point colour; DESIGN.md section 4, "YUV frames").
//
// The kernel is crop_device.h's body; this file is its two YUV sources, one template on whether a matrix is applied.  A tap's
// source pixel is frmap_yuv_pixel (three samples, converted and clipped to uint8 BEFORE they enter the resize sum) or, aligned,
// frmap_warp_pixel over it (the four corners converted first, then Pillow's float64 warp of rgb_pixel.h).
#include "crop_device.h"
#include "yuv_pixel.h"

static_assert(sizeof(FrmapYuvFrame) == 56, "FrmapYuvFrame is mirrored by resize.py and described in frmap_hip.h as 56 bytes");

template <bool ALIGN>
struct YuvSource {
  typedef FrmapYuvFrame Frame;
  static constexpr bool ROW_TAPS = false;
  FrmapYuvFetch px;
  int H, W;
  double m[ALIGN ? 6 : 1];
  __device__ __forceinline__ bool load(const Frame* __restrict__ frames, int n_frames, const FrmapRoi& r,
                                       const double* __restrict__ mats, int item, int) {
    if ((unsigned)r.frame >= (unsigned)n_frames) return false;
    px.f = frames[r.frame];
    if (!frmap_yuv_frame_ok(px.f)) return false;
    px.k = frmap_yuv_csc(px.f.csc);
    H = px.f.H;
    W = px.f.W;
    return !ALIGN || frmap_crop_load_matrix(mats, item, m);
  }
  __device__ __forceinline__ unsigned pixel(int x, int y) const { return ALIGN ? frmap_warp_pixel(H, W, m, x, y, px) : px(x, y); }
};

__global__ __launch_bounds__(256) void crop_resize_yuv_kernel(const FrmapYuvFrame* __restrict__ frames, int n_frames,
                                                              const FrmapRoi* __restrict__ rois, unsigned char* __restrict__ out,
                                                              int out_h, int out_w, int rows_per_block, int groups, int lds_rows,
                                                              int ksx_cap, int ksy_cap) {
  frmap_crop_body<YuvSource<false>>(frames, n_frames, rois, nullptr, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap,
                                    ksy_cap, 0);
}

__global__ __launch_bounds__(256) void align_crop_resize_yuv_kernel(const FrmapYuvFrame* __restrict__ frames, int n_frames,
                                                                    const FrmapRoi* __restrict__ rois, const double* __restrict__ mats,
                                                                    unsigned char* __restrict__ out, int out_h, int out_w,
                                                                    int rows_per_block, int groups, int lds_rows, int ksx_cap,
                                                                    int ksy_cap) {
  frmap_crop_body<YuvSource<true>>(frames, n_frames, rois, mats, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap,
                                   ksy_cap, 0);
}

extern "C" int frmap_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h,
                                     int out_w, int max_roi_h, int max_roi_w, void* stream) {
  return frmap_crop_launch("crop_resize_yuv", (const void*)crop_resize_yuv_kernel, false, frames, n_frames, rois, nullptr, out, N, out_h,
                           out_w, max_roi_h, max_roi_w, [&](const FrmapCropPlan& p, dim3 grid) {
                             hipLaunchKernelGGL(crop_resize_yuv_kernel, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream,
                                                (const FrmapYuvFrame*)frames, n_frames, (const FrmapRoi*)rois, out, out_h, out_w,
                                                p.rows_per_block, p.groups, p.lds_rows, p.ksx, p.ksy);
                           });
}

extern "C" int frmap_align_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out,
                                           int N, int out_h, int out_w, int max_roi_h, int max_roi_w, void* stream) {
  return frmap_crop_launch("align_crop_resize_yuv", (const void*)align_crop_resize_yuv_kernel, true, frames, n_frames, rois, mats, out, N,
                           out_h, out_w, max_roi_h, max_roi_w, [&](const FrmapCropPlan& p, dim3 grid) {
                             hipLaunchKernelGGL(align_crop_resize_yuv_kernel, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream,
                                                (const FrmapYuvFrame*)frames, n_frames, (const FrmapRoi*)rois, mats, out, out_h, out_w,
                                                p.rows_per_block, p.groups, p.lds_rows, p.ksx, p.ksy);
                           });
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
