// Face crops straight from device-resident packed frames (HWC uint8, RGB or BGR, rows possibly padded), the step between a
// detector's boxes and the embed batch in the reference's frame loop (src/app.py:224-236: `frame[y1:y2, x1:x2]` ->
// get_embedding's `[:, :, ::-1]` + `transforms.Resize((160, 160))`, :32-39): ROI crop + optional BGR -> RGB + Pillow-exact bilinear
// resize in one launch for every face of a detector.  The kernel is crop_device.h's body; this file is its two packed sources.
//
// Plain: a tap's source pixel is a byte triple of the frame.
//
// Eye-aligned: rotate about the point between the eyes, then crop the (margin) box, with no rotated frame in memory.  The
// reference's dataset step (src/data_prep.py:69-87, 144-150) rotates the whole image, crops and resizes, with cv2.warpAffine and
// cv2.resize.  DEPARTURE: the geometry is the reference's (angle, centre, "rotate the frame, then crop"), the RESAMPLING is
// Pillow's, which is what this project pins its image arithmetic to: crop i equals, bit for bit,
//     Image.fromarray(rgb_frame).rotate(angle_i, resample=Image.BILINEAR, center=center_i)      (same size, fill 0)
//          .crop((x1, y1, x2, y2)).resize((out_w, out_h), Image.BILINEAR)
// and not what cv2 would give (another interpolation grid and fixed-point weights).  A tap's source pixel is the ROTATED image's
// pixel at that position, computed on the spot by frmap_warp_pixel (rgb_pixel.h) from four pixels of the frame; see DESIGN.md
// section 4, "Aligned crops".  The host computes each face's output -> input matrix (frames.rotation_matrix); everything per
// pixel happens here.
#include "crop_device.h"

template <bool ALIGN>
struct PackedSource {
  typedef FrmapFrame Frame;
  static constexpr bool ROW_TAPS = !ALIGN;
  FrmapPackedFetch px;
  int H, W;
  double m[ALIGN ? 6 : 1];
  __device__ __forceinline__ bool load(const Frame* __restrict__ frames, int n_frames, const FrmapRoi& r,
                                       const double* __restrict__ mats, int item, int bgr) {
    if ((unsigned)r.frame >= (unsigned)n_frames) return false;
    const Frame f = frames[r.frame];
    px = FrmapPackedFetch{(const unsigned char*)f.base, f.pitch, bgr ? 2 : 0};
    H = f.H;
    W = f.W;
    return !ALIGN || frmap_crop_load_matrix(mats, item, m);
  }
  __device__ __forceinline__ unsigned pixel(int x, int y) const { return ALIGN ? frmap_warp_pixel(H, W, m, x, y, px) : px(x, y); }
  // The resampled taps of a plain crop, off a row pointer hoisted out of the loop with a wave-uniform `3 * t` added per tap, as the
  // kernel read them before the sources shared a body: through pixel(x + t, y) a 64-bit `(x + t) * 3` is paid per tap and lane,
  // and the kernel measured 9 % slower ("Frame kernels in one place").
  __device__ __forceinline__ void row_taps(int x, int y, int cnt, const int* k, FrmapResizeSum& s) const {
    const unsigned char* p = px.base + (size_t)y * px.pitch + (size_t)x * 3;
    const int c0 = px.c0, c2 = 2 - c0;
    for (int t = 0; t < cnt; ++t) s.tap(frmap_rgb_pack(p[3 * t + c0], p[3 * t + 1], p[3 * t + c2]), k[t]);
  }
};

__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const FrmapFrame* __restrict__ frames, int n_frames,
                                                             const FrmapRoi* __restrict__ rois, unsigned char* __restrict__ out,
                                                             int out_h, int out_w, int rows_per_block, int groups, int lds_rows,
                                                             int ksx_cap, int ksy_cap, int bgr) {
  frmap_crop_body<PackedSource<false>>(frames, n_frames, rois, nullptr, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap,
                                       ksy_cap, bgr);
}

__global__ __launch_bounds__(256) void align_crop_resize_u8_kernel(const FrmapFrame* __restrict__ frames, int n_frames,
                                                                   const FrmapRoi* __restrict__ rois, const double* __restrict__ mats,
                                                                   unsigned char* __restrict__ out, int out_h, int out_w,
                                                                   int rows_per_block, int groups, int lds_rows, int ksx_cap,
                                                                   int ksy_cap, int bgr) {
  frmap_crop_body<PackedSource<true>>(frames, n_frames, rois, mats, out, out_h, out_w, rows_per_block, groups, lds_rows, ksx_cap,
                                      ksy_cap, bgr);
}

extern "C" int frmap_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h,
                                    int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream) {
  return frmap_crop_launch("crop_resize_u8", (const void*)crop_resize_u8_kernel, false, frames, n_frames, rois, nullptr, out, N, out_h,
                           out_w, max_roi_h, max_roi_w, [&](const FrmapCropPlan& p, dim3 grid) {
                             hipLaunchKernelGGL(crop_resize_u8_kernel, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream,
                                                (const FrmapFrame*)frames, n_frames, (const FrmapRoi*)rois, out, out_h, out_w,
                                                p.rows_per_block, p.groups, p.lds_rows, p.ksx, p.ksy, bgr ? 1 : 0);
                           });
}

extern "C" int frmap_align_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out,
                                          int N, int out_h, int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream) {
  return frmap_crop_launch("align_crop_resize_u8", (const void*)align_crop_resize_u8_kernel, true, frames, n_frames, rois, mats, out, N,
                           out_h, out_w, max_roi_h, max_roi_w, [&](const FrmapCropPlan& p, dim3 grid) {
                             hipLaunchKernelGGL(align_crop_resize_u8_kernel, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream,
                                                (const FrmapFrame*)frames, n_frames, (const FrmapRoi*)rois, mats, out, out_h, out_w,
                                                p.rows_per_block, p.groups, p.lds_rows, p.ksx, p.ksy, bgr ? 1 : 0);
                           });
}

extern "C" int frmap_resize_coeffs_host(int in_size, int out_size, int32_t* bounds_out, int32_t* coeffs_out, int* ksize_out) {
  FRMAP_REQUIRE(in_size > 0 && out_size > 0, "resize_coeffs_host: sizes %d -> %d", in_size, out_size);
  FRMAP_REQUIRE((bounds_out != nullptr) == (coeffs_out != nullptr), "resize_coeffs_host: bounds_out and coeffs_out go together");
  const FrmapResizeAxis a = frmap_resize_axis(in_size, out_size);
  if (ksize_out) *ksize_out = a.ksize;
  if (!bounds_out) return 0;
  for (int xx = 0; xx < out_size; ++xx) {
    int32_t* k = coeffs_out + (size_t)xx * a.ksize;
    for (int x = 0; x < a.ksize; ++x) k[x] = 0;
    frmap_resize_taps(a, xx, &bounds_out[2 * xx], &bounds_out[2 * xx + 1], k);
  }
  return 0;
}

extern "C" int frmap_align_warp_host(const unsigned char* frame, int H, int W, long long pitch, const double* mat6, int x1, int y1,
                                     int x2, int y2, int bgr, unsigned char* out) {
  FRMAP_REQUIRE(frame && mat6 && out, "align_warp_host: null pointer");
  FRMAP_REQUIRE(H > 0 && W > 0 && pitch >= 3LL * W, "align_warp_host: frame %d x %d, pitch %lld", H, W, pitch);
  FRMAP_REQUIRE(x1 >= 0 && y1 >= 0 && x2 <= W && y2 <= H && x2 > x1 && y2 > y1,
                "align_warp_host: ROI (%d, %d, %d, %d) is empty or leaves its %dx%d frame", x1, y1, x2, y2, W, H);
  for (int i = 0; i < 6; ++i) FRMAP_REQUIRE(isfinite(mat6[i]), "align_warp_host: matrix entry %d is not finite", i);
  const FrmapPackedFetch px{frame, pitch, bgr ? 2 : 0};
  for (int y = y1; y < y2; ++y)
    for (int x = x1; x < x2; ++x)
      frmap_rgb_store3(out + ((size_t)(y - y1) * (x2 - x1) + (x - x1)) * 3, frmap_warp_pixel(H, W, mat6, x, y, px));
  return 0;
}
