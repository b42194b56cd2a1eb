// Face crops straight from device-resident frames: ROI crop + optional BGR -> RGB + Pillow-exact bilinear resize in one launch,
// the step between a detector's boxes and the embed batch in the reference's frame loop (src/app.py:224-236:
// `frame[y1:y2, x1:x2]` -> get_embedding's `[:, :, ::-1]` + `transforms.Resize((160, 160))`, :32-39).
//
// The integer arithmetic is resize.hip's (22-bit taps, accumulators started at 1 << 21, the horizontal result rounded to 8 bits
// in LDS before the vertical pass, an axis whose size is unchanged copied).  What differs: the source is a window of a pitched
// frame instead of a packed image, and the tap tables are not shipped by the host - a face box changes by a pixel or two every
// frame, so (input size, output size) pairs almost never repeat and a host table per pair costs more than the resize.  Each
// workgroup computes the taps it needs into LDS with the shared float64 function of resize_coeffs.h (all out_w columns, its own
// rows_per_block rows: a few thousand float64 operations), so the call needs nothing from the host but the ROI records.
#include "frame_records.h"
#include "frmap_common.h"
#include "resize_coeffs.h"

__device__ __forceinline__ int crop_clip8(int v) {
  v >>= FRMAP_RESIZE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const FrmapFrame* __restrict__ frames, int n_frames,
                                                             const FrmapRoi* __restrict__ rois, unsigned char* __restrict__ out,
                                                             int out_h, int out_w, int rows_per_block, int groups, int lds_rows,
                                                             int ksx_cap, int ksy_cap, int bgr) {
  extern __shared__ int s_mem[];
  unsigned* s_tmp = (unsigned*)s_mem;                 // [lds_rows][out_w] packed R | G << 8 | B << 16
  int* kx = s_mem + lds_rows * out_w;                 // [out_w][ksx_cap]
  int* bx = kx + out_w * ksx_cap;                     // [out_w][2] = (first input column, taps)
  int* ky = bx + 2 * out_w;                           // [rows_per_block][ksy_cap]
  int* by = ky + rows_per_block * ksy_cap;            // [rows_per_block][2]
  const int item = blockIdx.x / groups, grp = blockIdx.x - item * groups;
  const int y0 = grp * rows_per_block, y1 = min(y0 + rows_per_block, out_h), ny = y1 - y0;
  const FrmapRoi r = rois[item];
  // The ROI records are device data the host call never saw.  A record that breaks the contract, or is larger than the launch
  // was sized for, is not processed (its output stays unwritten): nothing is read outside a frame or written outside LDS.
  if ((unsigned)r.frame >= (unsigned)n_frames) return;
  const FrmapFrame f = frames[r.frame];
  if (r.x1 < 0 || r.y1 < 0 || r.x2 > f.W || r.y2 > f.H || r.x2 <= r.x1 || r.y2 <= r.y1) return;
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
  int row_first = y0, row_last = y1;                  // input rows (of the ROI) this block's output rows read
  if (ry) {
    row_first = by[0];
    row_last = by[2 * (ny - 1)] + by[2 * (ny - 1) + 1];
  }
  const int nrows = row_last - row_first;
  if (nrows > lds_rows) return;
  const unsigned char* src = (const unsigned char*)f.base + (size_t)r.y1 * f.pitch + (size_t)r.x1 * 3;
  const int c0 = bgr ? 2 : 0, c2 = 2 - c0;            // byte of a source pixel that holds R / B
  // ---- horizontal pass (ImagingResampleHorizontal_8bpc) over the needed rows
  for (int idx = threadIdx.x; idx < nrows * out_w; idx += 256) {
    const int rr = idx / out_w, xx = idx - rr * out_w;
    const unsigned char* rowp = src + (size_t)(row_first + rr) * f.pitch;
    unsigned v;
    if (rx) {
      const int xmin = bx[2 * xx], cnt = bx[2 * xx + 1];
      const int* k = kx + xx * ksx_cap;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      const unsigned char* p = rowp + (size_t)xmin * 3;
      for (int x = 0; x < cnt; ++x) {
        const int w = k[x];
        s0 += (int)p[3 * x + c0] * w; s1 += (int)p[3 * x + 1] * w; s2 += (int)p[3 * x + c2] * w;
      }
      v = (unsigned)crop_clip8(s0) | ((unsigned)crop_clip8(s1) << 8) | ((unsigned)crop_clip8(s2) << 16);
    } else {
      const unsigned char* p = rowp + (size_t)xx * 3;
      v = (unsigned)p[c0] | ((unsigned)p[1] << 8) | ((unsigned)p[c2] << 16);
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
      v = (unsigned)crop_clip8(s0) | ((unsigned)crop_clip8(s1) << 8) | ((unsigned)crop_clip8(s2) << 16);
    } else {
      v = s_tmp[j * out_w + xx];
    }
    unsigned char* o = dst + ((size_t)yy * out_w + xx) * 3;
    o[0] = (unsigned char)(v & 255u); o[1] = (unsigned char)((v >> 8) & 255u); o[2] = (unsigned char)((v >> 16) & 255u);
  }
}

extern "C" int frmap_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h,
                                    int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream) {
  FRMAP_REQUIRE(N >= 0, "crop_resize_u8: N = %d", N);
  if (N == 0) return 0;
  FRMAP_REQUIRE(frames && rois && out, "crop_resize_u8: null pointer");
  FRMAP_REQUIRE(n_frames > 0 && out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536 && max_roi_h > 0 && max_roi_w > 0 &&
                    max_roi_h <= (1 << 24) && max_roi_w <= (1 << 24),
                "crop_resize_u8: bad shape");
  const FrmapCropPlan p = frmap_crop_plan(out_h, out_w, max_roi_h, max_roi_w);
  FRMAP_REQUIRE(p.lds <= FRMAP_CROP_LDS_MAX, "crop_resize_u8: ROIs of up to %d x %d to %d x %d need %lld bytes of LDS for one output row (limit %d)",
                max_roi_h, max_roi_w, out_h, out_w, p.lds, FRMAP_CROP_LDS_MAX);
  FRMAP_REQUIRE((long long)N * p.groups <= 0x7fffffffLL, "crop_resize_u8: %d ROIs x %d row groups exceed the grid", N, p.groups);
  if (frmap_big_lds((const void*)crop_resize_u8_kernel, FRMAP_CROP_LDS_MAX)) return -2;
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(N * p.groups)), dim3(256), (size_t)p.lds, (hipStream_t)stream,
                     (const FrmapFrame*)frames, n_frames, (const FrmapRoi*)rois, out, out_h, out_w, p.rows_per_block, p.groups,
                     p.lds_rows, p.ksx, p.ksy, bgr ? 1 : 0);
  FRMAP_LAUNCH_CHECK();
  return 0;
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
