// The frame kernels in one place: ROI crop + Pillow-exact bilinear resize of regions of device-resident frames, one body for every
// kind of frame, and the one launcher of its entry points.  crop_resize.hip (packed frames) and yuv_crop.hip (4:2:0 frames) each
// instantiate it twice, plain and eye-aligned; DESIGN.md section 4, "Frame kernels in one place".
//
// The integer arithmetic is resize.hip's (22-bit taps, sums started at 1 << 21, the horizontal result rounded to 8 bits in LDS
// before the vertical pass, an axis whose size is unchanged copied).  What differs: the tap tables are not shipped by the host - a
// face box changes by a pixel or two every frame, so (input size, output size) pairs almost never repeat and a host table per
// pair costs more than the resize.  Each workgroup computes the taps it needs into LDS with the shared float64 function of
// resize_coeffs.h (all out_w columns, its own rows_per_block rows: a few thousand float64 operations), so a call needs nothing
// from the host but the records.  And a tap's source pixel comes from a Source:
//   typename Source::Frame                               the device record of a frame
//   bool load(frames, n_frames, roi, mats, item, bgr)    reads the ROI's frame record (and matrix) with the source's own guards;
//                                                        false = leave the output unwritten.  Uniform over the workgroup.
//   int H, W                                             the frame's size, valid after load
//   unsigned pixel(int x, int y) const                   R | G << 8 | B << 16 of frame pixel (x, y), uint8 BEFORE it enters a sum
//   static constexpr bool ROW_TAPS                       true: the source also has row_taps(x, y, cnt, k, sum), which adds the cnt taps
//                                                        pixel(x .. x + cnt - 1, y) * k[0 .. cnt) to `sum` its own way.  Only the
//                                                        packed plain source does (crop_resize.hip says why).
// The body tests the ROI after load() has returned: on an aligned crop the matrix is therefore read and tested BEFORE the ROI, where
// the kernels once tested the ROI first.  Every guard only returns, and matrix `item` exists for every item of the grid, so the
// records skipped and the memory read are the same.
// A pixel is recomputed by every tap that reads it (about two per pixel, whatever the scale) instead of being staged in LDS: the
// LDS need, and with it the launch shape and the supported reductions, are the same for every source.
#pragma once
#include "frame_records.h"
#include "frmap_common.h"
#include "resize_coeffs.h"

template <class Source>
__device__ __forceinline__ void frmap_crop_body(const typename Source::Frame* __restrict__ frames, int n_frames,
                                                const FrmapRoi* __restrict__ rois, const double* __restrict__ mats,
                                                unsigned char* __restrict__ out, int out_h, int out_w, int rows_per_block, int groups,
                                                int lds_rows, int ksx_cap, int ksy_cap, int bgr) {
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
  // than the launch was sized for, is not processed (its output stays unwritten): nothing is read outside a frame or written
  // outside LDS.  Every test is uniform over the workgroup, so all of its threads leave together.  (The ROI of an aligned crop
  // lies in the rotated frame, which has the frame's size.)
  Source src;
  if (!src.load(frames, n_frames, r, mats, item, bgr)) return;
  if (r.x1 < 0 || r.y1 < 0 || r.x2 > src.W || r.y2 > src.H || r.x2 <= r.x1 || r.y2 <= r.y1) return;
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
  // ---- horizontal pass (ImagingResampleHorizontal_8bpc) over the needed rows of the source
  for (int idx = threadIdx.x; idx < nrows * out_w; idx += 256) {
    const int rr = idx / out_w, xx = idx - rr * out_w;
    const int y = r.y1 + row_first + rr;
    unsigned v;
    if (rx) {
      const int xmin = r.x1 + bx[2 * xx], cnt = bx[2 * xx + 1];
      const int* k = kx + xx * ksx_cap;
      FrmapResizeSum s;
      if constexpr (Source::ROW_TAPS) {
        src.row_taps(xmin, y, cnt, k, s);
      } else {
        for (int x = 0; x < cnt; ++x) s.tap(src.pixel(xmin + x, y), k[x]);
      }
      v = s.pixel();
    } else {
      v = src.pixel(r.x1 + xx, y);
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
      FrmapResizeSum s;
      for (int y = 0; y < cnt; ++y) s.tap(s_tmp[(ymin + y) * out_w + xx], k[y]);
      v = s.pixel();
    } else {
      v = s_tmp[j * out_w + xx];
    }
    frmap_rgb_store3(dst + ((size_t)yy * out_w + xx) * 3, v);
  }
}

// Matrix `item` of `mats` into m[6]; false if an entry is not finite (the record is then skipped).
__device__ __forceinline__ bool frmap_crop_load_matrix(const double* __restrict__ mats, int item, double* m) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    m[i] = mats[(size_t)item * 6 + i];
    if (!__builtin_isfinite(m[i])) return false;
  }
  return true;
}

// What every entry point of the family does before and around its launch: the argument checks under the entry point's `name`,
// the launch shape from the size bounds (frmap_crop_plan), the opt-in to large LDS, and `launch(plan, grid)`, which starts
// `kernel` with the arguments of its own signature.  `need_mats`: the entry point takes matrices (float64 [N][6], 8-byte aligned).
template <class Launch>
int frmap_crop_launch(const char* name, const void* kernel, bool need_mats, const void* frames, int n_frames, const int32_t* rois,
                      const double* mats, unsigned char* out, int N, int out_h, int out_w, int max_roi_h, int max_roi_w,
                      Launch launch) {
  FRMAP_REQUIRE(N >= 0, "%s: N = %d", name, N);
  if (N == 0) return 0;
  FRMAP_REQUIRE(frames && rois && out && (mats || !need_mats), "%s: null pointer", name);
  FRMAP_REQUIRE(((uintptr_t)mats & 7) == 0, "%s: mats must be 8-byte aligned", name);
  // (the frame records start with uint64 plane addresses; the ROI records are int32; the output is byte-addressed)
  FRMAP_REQUIRE_ALIGNED_AS(name, frames, 8, "frames");
  FRMAP_REQUIRE_ALIGNED_AS(name, rois, 4, "rois");
  FRMAP_REQUIRE(n_frames > 0 && out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536 && max_roi_h > 0 && max_roi_w > 0 &&
                    max_roi_h <= (1 << 24) && max_roi_w <= (1 << 24),
                "%s: bad shape", name);
  const FrmapCropPlan p = frmap_crop_plan(out_h, out_w, max_roi_h, max_roi_w);
  FRMAP_REQUIRE(p.lds <= FRMAP_CROP_LDS_MAX, "%s: ROIs of up to %d x %d to %d x %d need %lld bytes of LDS for one output row (limit %d)",
                name, max_roi_h, max_roi_w, out_h, out_w, p.lds, FRMAP_CROP_LDS_MAX);
  FRMAP_REQUIRE((long long)N * p.groups <= 0x7fffffffLL, "%s: %d ROIs x %d row groups exceed the grid", name, N, p.groups);
  if (frmap_big_lds(kernel, FRMAP_CROP_LDS_MAX)) return -2;
  launch(p, dim3((unsigned)(N * p.groups)));
  FRMAP_LAUNCH_CHECK();
  return 0;
}
