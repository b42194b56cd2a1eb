// The frame loop's IoU tracker (the reference's process_webcam, src/app.py:126-147, 183-247) as one launch over many streams:
// every detection of a frame gets a face_id that survives from frame to frame by greedy IoU assignment against the boxes of the
// stream's previous frame, walked in the detector's order.  Per-stream state (previous raw boxes, their ids, next_id) stays on
// the device between steps; the step also emits the integer crop of every tracked box (frames.clip_boxes' rule), which is what
// the crop kernels cut.
//
// The rule is order-dependent - an earlier detection takes a previous box away from a later one - so one WAVEFRONT owns a stream
// and walks its detections one after the other, while the previous boxes are spread over the lanes: lane l holds previous boxes
// l, l + 64, l + 128, l + 192 (FRMAP_TRACK_MAX_BOXES = 256) with their ids and matched flags in registers.  Per detection every
// lane computes its IoUs (track_rule.h: float64, unfused), a __shfl_xor butterfly takes the wave's maximum, and a __ballot on
// equality with it per 64-box slot, lowest slot first, gives the lowest previous index among equal maxima - the reference's
// "first strict maximum".  The matched flag is set in the owning lane; next_id and the compaction of the new state are
// wave-uniform.  The whole old state is in registers before the first store of the new one, which goes in place.  No atomics, no
// traffic between workgroups, plain vector stores.
//
// Two DEPARTURES from the reference, stated in track_rule.h (a: float64 IoU) and here (b): the new state keeps only the boxes that
// received an id.  The reference rebuilds prev_boxes from every confident box but face_ids only from boxes that got an id, so a
// confident box whose crop is empty puts the two lists out of step (wrong ids later, or an IndexError its loop swallows with the
// frame); keeping them aligned differs from it in that case alone.
#include "frmap_common.h"
#include "track_rule.h"
#include "track_twin.h"

constexpr int TRACK_WAVES = 4;                            // streams per workgroup
constexpr int TRACK_SLOTS = FRMAP_TRACK_MAX_BOXES / 64;   // previous boxes per lane

__global__ __launch_bounds__(64 * TRACK_WAVES) void track_step_kernel(void* __restrict__ state, const float* __restrict__ boxes,
                                                                      const float* __restrict__ probs,
                                                                      const int32_t* __restrict__ counts,
                                                                      const int32_t* __restrict__ frame_hw, int n_streams,
                                                                      int max_boxes, float det_thresh, double iou_thresh,
                                                                      int32_t* __restrict__ ids_out, int32_t* __restrict__ rois_out) {
  __shared__ f32x4_t s_box[TRACK_WAVES][FRMAP_TRACK_MAX_BOXES];   // this step's raw boxes
  __shared__ int s_id[TRACK_WAVES][FRMAP_TRACK_MAX_BOXES];        // -1: skipped, -2: awaits its id, >= 0: its id
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * TRACK_WAVES + wave;
  const bool live = s < n_streams;                                // (wave-uniform; no early return: the barriers below are for all)
  const int sc = live ? s : 0;
  const size_t row = (size_t)sc * (size_t)max_boxes;
  // counts and the state's P are device data no host call ever saw: clamped, so no slot of another stream is touched
  int n = live ? counts[sc] : 0;
  n = n < 0 ? 0 : (n > max_boxes ? max_boxes : n);
  int32_t* meta = (int32_t*)state + 2 * sc;
  f32x4_t* st_box = (f32x4_t*)((char*)state + frmap_track_boxes_offset(n_streams)) + row;
  int32_t* st_id = (int32_t*)((char*)state + frmap_track_ids_offset(n_streams, max_boxes)) + row;
  int P = 0;
  unsigned next_id = 0u;
  if (live && n > 0) {
    P = meta[0];
    next_id = (unsigned)meta[1];
    P = P < 0 ? 0 : (P > max_boxes ? max_boxes : P);
  }
  // ---- the old state into registers: lane l holds previous boxes l + 64 k
  f32x4_t pbox[TRACK_SLOTS];
  int pid[TRACK_SLOTS];
  bool matched[TRACK_SLOTS];
#pragma unroll
  for (int k = 0; k < TRACK_SLOTS; ++k) {
    const int j = lane + 64 * k;
    pbox[k] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    pid[k] = 0;
    matched[k] = false;
    if (j < P) {
      pbox[k] = st_box[j];
      pid[k] = st_id[j];
    }
  }
  // ---- this step's boxes: skip rule and crop per box (independent of the order), staged in LDS for the walk
  const int H = live ? frame_hw[2 * sc] : 0, W = live ? frame_hw[2 * sc + 1] : 0;
  if (live) {
    for (int i = lane; i < max_boxes; i += 64) {
      int roi[4] = {0, 0, 0, 0};
      int tag = -1;
      if (i < n) {
        const f32x4_t b = *(const f32x4_t*)(boxes + 4 * (row + i));
        const float bb[4] = {b[0], b[1], b[2], b[3]};
        float pr = 0.f;
        if (probs) pr = probs[row + i];
        if (frmap_track_clip(bb, probs != nullptr, pr, det_thresh, H, W, roi)) tag = -2;
        else roi[0] = roi[1] = roi[2] = roi[3] = 0;
        s_box[wave][i] = b;
      }
      s_id[wave][i] = tag;
      *(int4*)(rois_out + 4 * (row + i)) = make_int4(roi[0], roi[1], roi[2], roi[3]);
    }
  }
  __syncthreads();
  // ---- the walk, in the detector's order
  const int pslots = (P + 63) >> 6;                               // (wave-uniform)
  for (int i = 0; i < n; ++i) {
    if (s_id[wave][i] == -1) continue;                            // (wave-uniform: every lane reads the same word)
    const f32x4_t b = s_box[wave][i];
    const float bb[4] = {b[0], b[1], b[2], b[3]};
    double iou[TRACK_SLOTS];
    double best = 0.0;                                            // a candidate must exceed 0 and the threshold
#pragma unroll
    for (int k = 0; k < TRACK_SLOTS; ++k) {
      iou[k] = 0.0;
      if (k < pslots) {
        const float pb[4] = {pbox[k][0], pbox[k][1], pbox[k][2], pbox[k][3]};
        const double v = frmap_track_iou(bb, pb);
        if (lane + 64 * k < P && !matched[k] && v > 0.0 && v > iou_thresh) iou[k] = v;
        if (iou[k] > best) best = iou[k];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double other = __shfl_xor(best, o, 64);
      if (other > best) best = other;
    }
    int id;
    if (best > 0.0) {                                             // (wave-uniform) the lowest index that holds the maximum
      int win = -1;
#pragma unroll
      for (int k = 0; k < TRACK_SLOTS; ++k) {
        const unsigned long long m = __ballot(iou[k] == best);
        if (win < 0 && m) win = 64 * k + (int)__builtin_ctzll(m);
      }
      int mine = 0;
#pragma unroll
      for (int k = 0; k < TRACK_SLOTS; ++k)
        if (win == lane + 64 * k) {
          matched[k] = true;
          mine = pid[k];
        }
      id = __shfl(mine, win & 63, 64);
    } else {
      id = (int)next_id;
      ++next_id;
    }
    if (lane == 0) s_id[wave][i] = id;
  }
  __syncthreads();
  // ---- ids out, and the new state: the boxes that got an id, in order
  if (live) {
    int kept = 0;
    for (int i0 = 0; i0 < max_boxes; i0 += 64) {
      const int i = i0 + lane;
      const int id = i < max_boxes ? s_id[wave][i] : -1;
      if (i < max_boxes) ids_out[row + i] = id;
      const bool has = i < n && id >= 0;
      const unsigned long long m = __ballot(has);
      if (has) {
        const int pos = kept + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        st_box[pos] = s_box[wave][i];
        st_id[pos] = id;
      }
      kept += __popcll(m);
    }
    if (n > 0 && lane == 0) {
      meta[0] = kept;
      meta[1] = (int)next_id;
    }
  }
}

extern "C" size_t frmap_track_state_bytes(int n_streams, int max_boxes) {
  if (n_streams < 0 || max_boxes < 1 || max_boxes > FRMAP_TRACK_MAX_BOXES) return 0;
  return frmap_track_bytes(n_streams, max_boxes);
}

extern "C" int frmap_track_step(void* state, const float* boxes, const float* probs, const int32_t* counts, const int32_t* frame_hw,
                                int n_streams, int max_boxes, double det_thresh, double iou_thresh, int32_t* ids_out,
                                int32_t* rois_out, void* stream) {
  FRMAP_REQUIRE(n_streams >= 0, "track_step: n_streams = %d", n_streams);
  FRMAP_REQUIRE(max_boxes >= 1 && max_boxes <= FRMAP_TRACK_MAX_BOXES, "track_step: max_boxes = %d is outside [1, %d]", max_boxes,
                FRMAP_TRACK_MAX_BOXES);
  if (n_streams == 0) return 0;
  FRMAP_REQUIRE(state && boxes && counts && frame_hw && ids_out && rois_out, "track_step: null pointer");
  FRMAP_REQUIRE((((uintptr_t)state | (uintptr_t)boxes | (uintptr_t)rois_out) & 15) == 0,
                "track_step: state, boxes and rois_out must be 16-byte aligned");
  FRMAP_REQUIRE_ALIGNED(probs, 4, "probs");
  FRMAP_REQUIRE_ALIGNED(counts, 4, "counts");
  FRMAP_REQUIRE_ALIGNED(frame_hw, 4, "frame_hw");
  FRMAP_REQUIRE_ALIGNED(ids_out, 4, "ids_out");
  FRMAP_REQUIRE(n_streams <= 0x7fffffff / FRMAP_TRACK_MAX_BOXES, "track_step: %d streams exceed the grid", n_streams);
  hipLaunchKernelGGL(track_step_kernel, dim3((unsigned)((n_streams + TRACK_WAVES - 1) / TRACK_WAVES)), dim3(64 * TRACK_WAVES), 0,
                     (hipStream_t)stream, state, boxes, probs, counts, frame_hw, n_streams, max_boxes, (float)det_thresh, iou_thresh,
                     ids_out, rois_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_track_step_host(void* state, const float* boxes, const float* probs, const int32_t* counts,
                                     const int32_t* frame_hw, int n_streams, int max_boxes, double det_thresh, double iou_thresh,
                                     int32_t* ids_out, int32_t* rois_out) {
  const char* why = frmap_track_step_twin(state, boxes, probs, counts, frame_hw, n_streams, max_boxes, det_thresh, iou_thresh, ids_out,
                                          rois_out);
  FRMAP_REQUIRE(!why, "track_step_host: %s (n_streams = %d, max_boxes = %d)", why, n_streams, max_boxes);
  return 0;
}
