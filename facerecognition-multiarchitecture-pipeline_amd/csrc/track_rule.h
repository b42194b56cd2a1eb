// The arithmetic of one IoU-tracker step (the reference's frame loop, src/app.py:126-147, 183-247), for the host and the device
// alike: the skip rule of a detection, its integer crop and the IoU of two raw boxes.  track.hip's kernel and the host twin
// (track_twin.h, frmap_track_step_host) run this text; a plain C++ compiler takes it too (tools/track_twin_check.cpp).  Not part
// of the public ABI.
//
// DEPARTURE (a) from the reference: the IoU is float64 arithmetic on the detector's float32 coordinates, every operation rounded
// once and nothing fused.  The reference mixes np.float32 rows with Python floats from tolist(), so which of its operations run in
// float32 depends on which operand a max() returned and on the NumPy major version; this is the same formula in the same order
// without that accident.  hipcc would contract a1 + a2 - inter and the area products into FMAs on the device, so frmap_track_iou -
// the one function here with arithmetic that could be fused - turns contraction off; the division is the correctly rounded default (the library is not built with fast-math).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRMAP_TRACK_HD __host__ __device__
#else
#define FRMAP_TRACK_HD
#endif

constexpr int FRMAP_TRACK_MAX_BOXES = 256;   // per stream: four previous boxes per lane of a wavefront

// Python's max(a, b) / min(a, b): the first operand unless the second is strictly greater / smaller
FRMAP_TRACK_HD inline double frmap_track_max(double a, double b) { return b > a ? b : a; }
FRMAP_TRACK_HD inline double frmap_track_min(double a, double b) { return b < a ? b : a; }

// calc_iou (app.py:126-147) of two raw boxes (x1, y1, x2, y2): intersection corners by max / min, 0 when they cross, else
// inter / (a1 + a2 - inter) if that union is positive, else 0
FRMAP_TRACK_HD inline double frmap_track_iou(const float* a, const float* b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3];
  const double bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  const double x_left = frmap_track_max(ax1, bx1), y_top = frmap_track_max(ay1, by1);
  const double x_right = frmap_track_min(ax2, bx2), y_bottom = frmap_track_min(ay2, by2);
  if (x_right < x_left || y_bottom < y_top) return 0.0;
  const double inter = (x_right - x_left) * (y_bottom - y_top);
  const double area_a = (ax2 - ax1) * (ay2 - ay1);
  const double area_b = (bx2 - bx1) * (by2 - by1);
  const double uni = area_a + area_b - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

// min(hi, max(0, int(v))) for a finite v without ever converting a value outside int's range: int() truncates toward zero, so
// every v < 1 clamps to 0 and every v >= hi to hi (the comparison is exact in float64, whatever hi)
FRMAP_TRACK_HD inline int frmap_track_coord(float v, int hi) {
  const double d = v;
  if (d >= (double)hi) return hi;
  return d <= 0.0 ? 0 : (int)d;
}

// The skip rule and the integer crop of one detection (frames.clip_boxes; app.py:190-200): skipped (false) when its probability
// is below det_thresh IN FLOAT32 (has_prob false: every box is confident), when a coordinate or the probability is not finite,
// or when the crop is empty; otherwise roi = the crop, 0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H.  clip_boxes clamps x1 / y1 only
// from below and x2 / y2 only from above; clamping all four to [0, W] / [0, H] changes neither the verdict (an x1 beyond W or an
// x2 below 0 leaves x2 <= x1 either way) nor a kept crop.
FRMAP_TRACK_HD inline bool frmap_track_clip(const float* box, bool has_prob, float prob, float det_thresh, int H, int W, int* roi) {
  if (has_prob && !(__builtin_isfinite(prob) && !(prob < det_thresh))) return false;
  if (!(__builtin_isfinite(box[0]) && __builtin_isfinite(box[1]) && __builtin_isfinite(box[2]) && __builtin_isfinite(box[3]))) return false;
  if (H <= 0 || W <= 0) return false;
  const int x1 = frmap_track_coord(box[0], W), y1 = frmap_track_coord(box[1], H);
  const int x2 = frmap_track_coord(box[2], W), y2 = frmap_track_coord(box[3], H);
  if (x2 <= x1 || y2 <= y1) return false;
  roi[0] = x1; roi[1] = y1; roi[2] = x2; roi[3] = y2;
  return true;
}

// State buffer of n_streams streams of up to max_boxes boxes (frmap_track_state_bytes; all-zero bytes = fresh):
//   int32   meta [n_streams][2]             = (P = boxes of the previous step, next_id)     at byte 0
//   float32 boxes[n_streams][max_boxes][4]  raw (x1, y1, x2, y2), the first P valid          at byte align16(8 * n_streams)
//   int32   ids  [n_streams][max_boxes]     their ids                                        right after the boxes
FRMAP_TRACK_HD inline size_t frmap_track_boxes_offset(int n_streams) { return ((size_t)8 * (size_t)n_streams + 15) & ~(size_t)15; }
FRMAP_TRACK_HD inline size_t frmap_track_ids_offset(int n_streams, int max_boxes) {
  return frmap_track_boxes_offset(n_streams) + (size_t)16 * (size_t)n_streams * (size_t)max_boxes;
}
FRMAP_TRACK_HD inline size_t frmap_track_bytes(int n_streams, int max_boxes) {
  return frmap_track_ids_offset(n_streams, max_boxes) + (size_t)4 * (size_t)n_streams * (size_t)max_boxes;
}
