// What the frame kernels (crop_device.h's body; crop_resize.hip, yuv_crop.hip) share: the device records they take - frames and regions
// of interest - and the launch shape all derive from the size bounds of a call.  Not part of the public ABI as types - include/frmap_hip.h
// states the records' layout in words.
#pragma once

struct FrmapFrame {            // mirrored by resize.py (24 bytes)
  unsigned long long base;     // device address of pixel (0, 0); HWC uint8, 3 bytes per pixel
  int H, W;
  long long pitch;             // bytes from one row to the next, >= 3 * W
};
struct FrmapYuvFrame {         // mirrored by resize.py (56 bytes): one 4:2:0 frame of 8-bit samples (yuv_pixel.h has the rule)
  unsigned long long y, u, v;  // device addresses of sample (0, 0) of each plane; chroma planes are ceil(H/2) x ceil(W/2)
  int H, W;
  long long y_pitch, c_pitch;  // bytes from one row to the next: >= W, >= c_step * ceil(W/2)
  int c_step;                  // bytes from one chroma sample to the next in its row: 1 = planar (I420, YV12), 2 = interleaved
  int csc;                     // row of the conversion table: 0 bt601 limited, 1 bt601 full, 2 bt709 limited, 3 bt709 full
};                             // NV12: v = u + 1, c_step = 2; NV21: u = v + 1, c_step = 2
struct FrmapRoi {              // mirrored by resize.py (20 bytes)
  int frame, x1, y1, x2, y2;   // rows [y1, y2), columns [x1, x2) of frames[frame]
};

constexpr int FRMAP_CROP_LDS_MAX = 160 * 1024;

// Launch shape from the size bounds alone.  ceil(max(scale, 1)) per axis gives the tap count 2 c + 1; the input rows r output
// rows touch at scale s are at most ceil(r s) + 2 ceil(max(s, 1)) + 2 (and never more than the ROI has).  One workgroup resizes
// rows_per_block output rows: 8, fewer when the input rows those touch would not fit 64 KB of LDS (two workgroups per CU).
struct FrmapCropPlan {
  int rows_per_block, groups, lds_rows, ksx, ksy;
  long long lds;               // bytes of LDS per workgroup; the caller rejects a plan beyond FRMAP_CROP_LDS_MAX
};
inline FrmapCropPlan frmap_crop_plan(int out_h, int out_w, int max_roi_h, int max_roi_w) {
  const long long cx = max_roi_w > out_w ? (max_roi_w + out_w - 1) / out_w : 1, cy = max_roi_h > out_h ? (max_roi_h + out_h - 1) / out_h : 1;
  const long long ksx = 2 * cx + 1, ksy = 2 * cy + 1;
  auto window = [&](long long r) {
    const long long w = (r * max_roi_h + out_h - 1) / out_h + 2 * cy + 2;
    return w < max_roi_h ? w : (long long)max_roi_h;
  };
  auto lds_bytes = [&](long long r) { return 4 * (window(r) * out_w + out_w * (ksx + 2) + r * (ksy + 2)); };
  int rows_per_block = out_h < 8 ? out_h : 8;
  while (rows_per_block > 1 && lds_bytes(rows_per_block) > 64 * 1024) rows_per_block /= 2;
  FrmapCropPlan p;
  p.rows_per_block = rows_per_block;
  p.groups = (out_h + rows_per_block - 1) / rows_per_block;
  p.lds_rows = (int)window(rows_per_block);
  p.ksx = (int)ksx;
  p.ksy = (int)ksy;
  p.lds = lds_bytes(rows_per_block);
  return p;
}
