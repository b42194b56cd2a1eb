// Track templates: the embeddings of a track (the tracker's face_id, track.hip) pooled on the device into a decayed sum and a
// weight per track, and every embedding row of the step answered with its track's template sum / weight.  The rule is
// frames.fuse_tracks; its arithmetic and the state layout are track_fuse_rule.h.  One launch per step over all streams, between
// the model and the match; the state stays on the device and mirrors the tracker's state slot for slot: after a step a stream's
// slots are the detections that received an id, in detection order.
//
// One WORKGROUP of four wavefronts owns a stream.  The slot of a track moves whenever the detector's order changes, so an update
// in place would overwrite sums other faces still have to read: every stream has two banks of slots, a step reads the current one
// and writes the other, and the stream's own meta word says which is current - flipped by one thread after the workgroup's
// barrier.  The step's ids, the old bank's ids and the row of every detection are staged in LDS; wave 0 turns `id >= 0` into slot
// positions with a ballot prefix; then the waves take the stream's faces in turn: the lanes find the face's old slot with a ballot
// over the at most 256 old ids, test the row for non-finite values, and stream old sum, row and new sum through float4 accesses
// (dim a multiple of 4; otherwise element by element).  Rows that are only passed through - id -1, no such detection, or the loser
// of two rows that name one detection - are copied by the wave that meets them in the scan of `rows`.  No atomics, no traffic between workgroups, plain vector stores.
//
// `counts`, `ids`, `rows` and the state's meta words are device data no host call ever saw: counts and P are clamped, a row takes
// part in a stream's update only if it names a detection below the clamped count, and every index into the state is below
// max_boxes - so whatever they hold, a workgroup touches its own stream's slots, and rows of `fused` / `frames_out` below n_rows.
#include "frmap_common.h"
#include "track_fuse_rule.h"
#include "track_fuse_twin.h"

constexpr int FUSE_WAVES = 4;                              // wavefronts per workgroup = faces of a stream in flight

// dst[0 .. dim) = src[0 .. dim) bit for bit (a NaN keeps its payload), by one wavefront; dv = the part moved as 16-byte pieces
__device__ __forceinline__ void fuse_copy_row(const float* __restrict__ src, float* __restrict__ dst, int dim, int dv, int lane) {
  for (int k = lane * 4; k < dv; k += 256) *(u32x4_t*)(dst + k) = *(const u32x4_t*)(src + k);
  for (int k = dv + lane; k < dim; k += 64) ((uint32_t*)dst)[k] = ((const uint32_t*)src)[k];
}

__global__ __launch_bounds__(64 * FUSE_WAVES) void track_fuse_kernel(void* state, const int32_t* __restrict__ ids,
                                                                     const int32_t* __restrict__ counts,
                                                                     const float* __restrict__ emb, const int32_t* __restrict__ rows,
                                                                     int n_rows, int n_streams, int max_boxes, int dim, float decay,
                                                                     float* __restrict__ fused, float* __restrict__ frames_out) {
  __shared__ int s_old[FRMAP_TRACK_MAX_BOXES];             // ids of the current bank, -1 beyond P
  __shared__ int s_new[FRMAP_TRACK_MAX_BOXES];             // this step's ids, -1 beyond n
  __shared__ int s_row[FRMAP_TRACK_MAX_BOXES];             // the row of detection i, -1: none
  __shared__ int s_pos[FRMAP_TRACK_MAX_BOXES];             // its slot in the new bank (where its id >= 0)
  __shared__ int s_kept;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s = blockIdx.x;                                // (the grid is n_streams workgroups)
  int n = counts[s];
  n = n < 0 ? 0 : (n > max_boxes ? max_boxes : n);
  int32_t* meta = (int32_t*)state + 2 * s;
  int32_t* st_id = (int32_t*)((char*)state + frmap_fuse_ids_offset(n_streams));
  float* st_w = (float*)((char*)state + frmap_fuse_w_offset(n_streams, max_boxes));
  float* st_sum = (float*)((char*)state + frmap_fuse_sum_offset(n_streams, max_boxes));
  const size_t pitch = frmap_fuse_pitch(dim);
  const int dv = (dim & 3) == 0 ? dim : 0;                 // elements that go as float4; the rest one by one
  int P = 0, bank = 0;
  if (n > 0) {
    P = meta[0];
    P = P < 0 ? 0 : (P > max_boxes ? max_boxes : P);
    bank = meta[1] & 1;
  }
  const size_t old0 = frmap_fuse_slot(s, bank, 0, max_boxes);
  // ---- the step's ids and the old bank's ids into LDS (256 threads, at most 256 slots)
  s_row[tid] = -1;
  s_new[tid] = tid < n ? ids[(size_t)s * (size_t)max_boxes + (size_t)tid] : -1;
  s_old[tid] = tid < P ? st_id[old0 + (size_t)tid] : -1;
  __syncthreads();
  // ---- slot positions: a ballot prefix over id >= 0, by wave 0
  if (wave == 0) {
    int kept = 0;
    for (int i0 = 0; i0 < max_boxes; i0 += 64) {
      const int i = i0 + lane;                             // (< 256)
      const bool has = s_new[i] >= 0;
      const unsigned long long m = __ballot(has);
      s_pos[i] = kept + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      kept += __popcll(m);
    }
    if (lane == 0) s_kept = kept;
  }
  // ---- the rows: which detection of this stream each belongs to
  for (int r = tid; r < n_rows; r += 64 * FUSE_WAVES) {
    const int2 sd = ((const int2*)rows)[r];
    if (sd.x == s && sd.y >= 0 && sd.y < n) s_row[sd.y] = r;
  }
  __syncthreads();
  // ---- a row that only passes through is copied by the wave that meets it here: its detection has no id, it names no detection
  // at all, or - two rows that name the same detection, which the host entries refuse - it lost s_row to the other row.  A row
  // whose stream field is no stream falls to workgroup 0, so every row of `fused` is written whatever `rows` holds.
  for (int r0 = wave * 64; r0 < n_rows; r0 += 64 * FUSE_WAVES) {
    const int r = r0 + lane;
    bool pass = false;
    if (r < n_rows) {
      const int2 sd = ((const int2*)rows)[r];
      const bool stream_ok = sd.x >= 0 && sd.x < n_streams;
      const bool mine = stream_ok ? sd.x == s : s == 0;
      const bool valid = stream_ok && sd.x == s && sd.y >= 0 && sd.y < n;
      pass = mine && !(valid && s_new[sd.y] >= 0 && s_row[sd.y] == r);
    }
    unsigned long long m = __ballot(pass);
    while (m) {                                            // (wave-uniform)
      const int rr = r0 + (int)__builtin_ctzll(m);
      m &= m - 1;
      fuse_copy_row(emb + (size_t)rr * (size_t)dim, fused + (size_t)rr * (size_t)dim, dim, dv, lane);
      if (lane == 0) frames_out[rr] = 0.f;
    }
  }
  if (n == 0) return;                                      // (the whole workgroup) tracks survive a frame without detections
  // ---- the faces, one wavefront each in turn
  const int pchunks = (P + 63) >> 6;
  for (int i = wave; i < n; i += FUSE_WAVES) {
    const int id = s_new[i];                               // (wave-uniform: every lane reads the same word)
    if (id < 0) continue;
    const int r = s_row[i];
    int j = -1;                                            // the track's slot in the old bank: the lowest one that holds its id
    for (int k = 0; k < pchunks && j < 0; ++k) {
      const unsigned long long m = __ballot(s_old[64 * k + lane] == id);
      if (m) j = 64 * k + (int)__builtin_ctzll(m);
    }
    const float* e = emb + (size_t)(r < 0 ? 0 : r) * (size_t)dim;
    float* fo = fused + (size_t)(r < 0 ? 0 : r) * (size_t)dim;
    bool bad = false;
    if (r >= 0) {
      for (int k = lane * 4; k < dv; k += 256) {
        const u32x4_t u = *(const u32x4_t*)(e + k);
        bad |= !(frmap_fuse_finite_bits(u[0]) && frmap_fuse_finite_bits(u[1]) && frmap_fuse_finite_bits(u[2]) && frmap_fuse_finite_bits(u[3]));
      }
      for (int k = dv + lane; k < dim; k += 64) bad |= !frmap_fuse_finite_bits(((const uint32_t*)e)[k]);
    }
    const bool finite = r >= 0 && __ballot(bad) == 0ull;   // (wave-uniform)
    const bool had = j >= 0;
    const float wo = had ? st_w[old0 + (size_t)j] : 0.f;
    const float w2 = finite ? (had ? frmap_fuse_acc(decay, wo, 1.f) : 1.f) : wo;
    const bool emit = finite && !(w2 == 0.f);
    const size_t dst = frmap_fuse_slot(s, bank ^ 1, s_pos[i], max_boxes);
    const float* so = st_sum + (old0 + (size_t)(had ? j : 0)) * pitch;
    float* sn = st_sum + dst * pitch;
    for (int k = lane * 4; k < dv; k += 256) {
      f32x4_t ev = (f32x4_t){0.f, 0.f, 0.f, 0.f}, sv = ev, nv;
      if (finite) ev = *(const f32x4_t*)(e + k);
      if (had) sv = *(const f32x4_t*)(so + k);
      if (finite && had) {
#pragma unroll
        for (int c = 0; c < 4; ++c) nv[c] = frmap_fuse_acc(decay, sv[c], ev[c]);
      } else {
        nv = finite ? ev : sv;                             // a new track takes the row; without a row the old slot is carried over
      }
      *(f32x4_t*)(sn + k) = nv;
      if (emit) {
        f32x4_t q;
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = frmap_fuse_mean(nv[c], w2);
        *(f32x4_t*)(fo + k) = q;
      }
    }
    for (int k = dv + lane; k < dim; k += 64) {
      const float ev = finite ? e[k] : 0.f, sv = had ? so[k] : 0.f;
      const float nv = finite && had ? frmap_fuse_acc(decay, sv, ev) : (finite ? ev : sv);
      sn[k] = nv;
      if (emit) fo[k] = frmap_fuse_mean(nv, w2);
    }
    if (r >= 0 && !emit) fuse_copy_row(e, fo, dim, dv, lane);   // a non-finite row goes back as it came
    if (lane == 0) {
      st_id[dst] = id;
      st_w[dst] = w2;
      if (r >= 0) frames_out[r] = emit ? w2 : 0.f;
    }
  }
  __syncthreads();                                         // every slot of the new bank is on its way before the bank flips
  if (tid == 0) {
    meta[0] = s_kept;
    meta[1] = bank ^ 1;
  }
}

extern "C" size_t frmap_track_fuse_state_bytes(int n_streams, int max_boxes, int dim) {
  if (n_streams < 0 || max_boxes < 1 || max_boxes > FRMAP_TRACK_MAX_BOXES || dim < 1 || dim > FRMAP_TRACK_FUSE_MAX_DIM) return 0;
  return frmap_fuse_bytes(n_streams, max_boxes, dim);
}

extern "C" int frmap_track_fuse(void* state, const int32_t* ids, const int32_t* counts, const float* emb, const int32_t* rows,
                                int n_rows, int n_streams, int max_boxes, int dim, float decay, float* fused, float* frames_out,
                                void* stream) {
  FRMAP_REQUIRE(n_streams >= 0, "track_fuse: n_streams = %d", n_streams);
  FRMAP_REQUIRE(max_boxes >= 1 && max_boxes <= FRMAP_TRACK_MAX_BOXES, "track_fuse: max_boxes = %d is outside [1, %d]", max_boxes,
                FRMAP_TRACK_MAX_BOXES);
  FRMAP_REQUIRE(dim >= 1 && dim <= FRMAP_TRACK_FUSE_MAX_DIM, "track_fuse: dim = %d is outside [1, %d]", dim, FRMAP_TRACK_FUSE_MAX_DIM);
  FRMAP_REQUIRE(decay > 0.f && decay <= 1.f, "track_fuse: decay = %g is outside (0, 1]", (double)decay);
  FRMAP_REQUIRE(n_rows >= 0 && (long long)n_rows <= (long long)n_streams * max_boxes,
                "track_fuse: n_rows = %d for %d streams of %d boxes", n_rows, n_streams, max_boxes);
  if (n_streams == 0) return 0;
  FRMAP_REQUIRE(state && ids && counts, "track_fuse: null pointer");
  FRMAP_REQUIRE(n_rows == 0 || (emb && rows && fused && frames_out), "track_fuse: null pointer");
  FRMAP_REQUIRE(emb != fused || n_rows == 0, "track_fuse: fused must not be emb");
  FRMAP_REQUIRE((((uintptr_t)state | (uintptr_t)emb | (uintptr_t)fused) & 15) == 0 && ((uintptr_t)rows & 7) == 0,
                "track_fuse: state, emb and fused must be 16-byte aligned, rows 8-byte aligned");
  FRMAP_REQUIRE_ALIGNED(ids, 4, "ids");
  FRMAP_REQUIRE_ALIGNED(counts, 4, "counts");
  FRMAP_REQUIRE_ALIGNED(frames_out, 4, "frames_out");
  FRMAP_REQUIRE(n_streams <= 0x7fffffff / FRMAP_TRACK_MAX_BOXES, "track_fuse: %d streams exceed the grid", n_streams);
  hipLaunchKernelGGL(track_fuse_kernel, dim3((unsigned)n_streams), dim3(64 * FUSE_WAVES), 0, (hipStream_t)stream, state, ids, counts,
                     emb, rows, n_rows, n_streams, max_boxes, dim, decay, fused, frames_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_track_fuse_host(void* state, const int32_t* ids, const int32_t* counts, const float* emb, const int32_t* rows,
                                     int n_rows, int n_streams, int max_boxes, int dim, float decay, float* fused,
                                     float* frames_out) {
  const char* why = frmap_track_fuse_twin(state, ids, counts, emb, rows, n_rows, n_streams, max_boxes, dim, decay, fused, frames_out);
  FRMAP_REQUIRE(!why, "track_fuse_host: %s (n_rows = %d, n_streams = %d, max_boxes = %d, dim = %d)", why, n_rows, n_streams, max_boxes,
                dim);
  return 0;
}
