// The classification tally: one launch per batch reads logits and labels and adds exact integers into a small device-resident
// state - rows, correct, fixed-point loss, rank histogram, per-class support / predicted / hit, calibration bins, confusion
// matrix - so an evaluation copies nothing to the host and synchronises once, at the end (evaluate.ClassificationTally,
// evaluate.evaluate_stream; the accumulate step of src/testing.py:278-283 and the metric block of src/advanced_metrics.py).
// The rule, the state layout and the overflow reach of the fixed-point sums are tally_rule.h; evaluate.tally_rule states
// the same in numpy.
//
// One WAVEFRONT per row, lanes strided over C, four wavefronts a workgroup, the workgroups striding over the rows.  The label and
// z[y] are read first; one pass over the row gives the maximum, the first arg-max, the two rank counts and the finiteness test
// (an integer test on the exponent bits); a second pass sums exp(z - max) lane by lane, then across the lanes by an xor
// butterfly (32, 16, ... 1), which leaves every lane with the same bits.  The row's adds outside the header go out as ONE vector
// 64-bit atomic instruction: lane k issues add k of frmap_tally_row_add - held back one row, so that a wavefront whose next row
// adds to the same word (a long batch of one class, one prediction, one bin) sums in a register first.  The five header counters are summed per wavefront in
// registers over all its rows, per workgroup through LDS, and reach the state as at most five atomics per workgroup - a batch
// of one class does not queue one atomic per row on `rows`.  Integer adds only: a state is the same bits for any order of the
// rows and any split into launches.  Every row is addressed as pointer + (size_t) r * C, every cell of the matrix as
// (size_t) y * C + pred.
#include "frmap_common.h"
#include "tally_rule.h"
#include "tally_twin.h"

constexpr int TALLY_WAVES = 4;            // rows in flight per workgroup
constexpr int TALLY_LOADS = 8;            // loads a lane keeps in flight on a wide row (8 x 64 columns a round)
constexpr int TALLY_MAX_BLOCKS = 2048;    // 8 per compute unit of 256 (5 are resident at 82 VGPRs); beyond that a wavefront takes several rows

__device__ __forceinline__ void tally_add(uint64_t* p, uint64_t v) {
  __hip_atomic_fetch_add((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64 * TALLY_WAVES) void classify_tally_kernel(const float* __restrict__ logits,
                                                                          const int32_t* __restrict__ labels, int B, int C, int R,
                                                                          int n_bins, int keep_confusion, uint64_t* state,
                                                                          int32_t* __restrict__ row_pred, int32_t* __restrict__ row_rank,
                                                                          float* __restrict__ row_conf, float* __restrict__ row_loss) {
  __shared__ unsigned long long s_head[TALLY_WAVES][5];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  unsigned long long head[5] = {0ull, 0ull, 0ull, 0ull, 0ull};   // rows, ignored, nonfinite, correct, loss_q of this wavefront (wave-uniform)
  size_t pend_word = 0;                  // lane k < 8: add k of the previous row, held back while the next row adds to the same word
  uint64_t pend_amount = 0;              // (word 0 is a header word: no row add ever names it)
  for (long long r = (long long)blockIdx.x * TALLY_WAVES + wave; r < (long long)B; r += (long long)gridDim.x * TALLY_WAVES) {
    const int y = labels[r];
    int pred = -1, rank = -1;
    float conf = __builtin_nanf(""), loss = __builtin_nanf("");
    bool counted = false;
    if (y < 0 || y >= C) {
      head[FRMAP_TALLY_IGNORED] += 1;
    } else {
      const float* z = logits + (size_t)r * (size_t)C;
      const float zy = z[y];
      float mx = -INFINITY;
      int mi = 0x7FFFFFFF, above = 0;
      bool bad = false;
      auto see = [&](float v, int c) {
        bad |= !frmap_tally_finite_bits(__float_as_uint(v));
        if (v > mx || (v == mx && c < mi)) { mx = v; mi = c; }
        above += (v > zy || (c < y && v == zy)) ? 1 : 0;
      };
      // a wide row is one wavefront's alone, so its loads go out TALLY_LOADS at a time (all below C) and are used in column order
      int c = lane;
      for (; c + 64 * (TALLY_LOADS - 1) < C; c += 64 * TALLY_LOADS) {
        float v[TALLY_LOADS];
#pragma unroll
        for (int k = 0; k < TALLY_LOADS; ++k) v[k] = z[c + 64 * k];
#pragma unroll
        for (int k = 0; k < TALLY_LOADS; ++k) see(v[k], c + 64 * k);
      }
      for (; c < C; c += 64) see(z[c], c);
      if (__ballot(bad) != 0ull) {                         // (wave-uniform)
        head[FRMAP_TALLY_NONFINITE] += 1;
      } else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(mx, o, 64);
          const int oi = __shfl_xor(mi, o, 64);
          if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
          above += __shfl_xor(above, o, 64);
        }
        float sum = 0.f;
        c = lane;                                          // (the same order of additions as one column at a time)
        for (; c + 64 * (TALLY_LOADS - 1) < C; c += 64 * TALLY_LOADS) {
          float v[TALLY_LOADS];
#pragma unroll
          for (int k = 0; k < TALLY_LOADS; ++k) v[k] = z[c + 64 * k];
#pragma unroll
          for (int k = 0; k < TALLY_LOADS; ++k) sum += expf(v[k] - mx);
        }
        for (; c < C; c += 64) sum += expf(z[c] - mx);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        pred = mi;
        rank = above;
        conf = 1.0f / sum;
        loss = fmaxf(0.f, logf(sum) + (mx - zy));
        counted = true;
      }
    }
    if (lane == 0) {
      if (row_pred) row_pred[r] = pred;
      if (row_rank) row_rank[r] = rank;
      if (row_conf) row_conf[r] = conf;
      if (row_loss) row_loss[r] = loss;
    }
    if (!counted) continue;                                // (wave-uniform)
    head[FRMAP_TALLY_ROWS] += 1;
    head[FRMAP_TALLY_CORRECT] += rank == 0 ? 1 : 0;
    head[FRMAP_TALLY_LOSS_Q] += frmap_tally_loss_q(loss);
    // the bin: the edges at or below conf, counted lane by lane (frmap_tally_bin is the serial count)
    int at_or_below = 0;
    const double cd = (double)conf;
    for (int k = lane; k < n_bins; k += 64) at_or_below += frmap_tally_edge(k, n_bins) <= cd ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) at_or_below += __shfl_xor(at_or_below, o, 64);
    const int bin = at_or_below - 1;                       // (>= 0: edge 0 is 0 and conf >= 1 / C)
    if (lane < FRMAP_TALLY_ROW_ADDS) {
      size_t word;
      uint64_t amount;
      frmap_tally_row_add(lane, C, R, n_bins, keep_confusion, y, pred, rank, bin, frmap_tally_conf_q(conf), &word, &amount);
      if (amount) {
        if (word == pend_word) {
          pend_amount += amount;
        } else {
          if (pend_amount) tally_add(state + pend_word, pend_amount);
          pend_word = word;
          pend_amount = amount;
        }
      }
    }
  }
  if (pend_amount) tally_add(state + pend_word, pend_amount);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s_head[wave][k] = head[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < TALLY_WAVES; ++w) v += s_head[w][threadIdx.x];
    if (v) tally_add(state + threadIdx.x, v);              // (words 0 .. 4 of the header, in the order of `head`)
  }
}

extern "C" size_t frmap_classify_tally_words(int C, int R, int n_bins, int keep_confusion) {
  if (!frmap_tally_shape_ok(C, R, n_bins, keep_confusion)) return 0;
  return frmap_tally_words(C, R, n_bins, keep_confusion);
}

extern "C" int frmap_classify_tally(const float* logits, const int32_t* labels, int B, int C, int R, int n_bins, int keep_confusion,
                                    uint64_t* state, int32_t* row_pred_out, int32_t* row_rank_out, float* row_conf_out,
                                    float* row_loss_out, void* stream) {
  FRMAP_REQUIRE(B >= 1, "classify_tally: B = %d is below 1", B);
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "classify_tally: B = %d rows exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  FRMAP_REQUIRE(C >= 1, "classify_tally: C = %d is below 1", C);
  FRMAP_REQUIRE(R >= 1 && R <= FRMAP_TALLY_MAX_RANKS, "classify_tally: R = %d is outside [1, %d]", R, FRMAP_TALLY_MAX_RANKS);
  FRMAP_REQUIRE(n_bins >= 1 && n_bins <= FRMAP_TALLY_MAX_BINS, "classify_tally: n_bins = %d is outside [1, %d]", n_bins,
                FRMAP_TALLY_MAX_BINS);
  FRMAP_REQUIRE(!(keep_confusion && C > FRMAP_TALLY_MAX_CONFUSION_C),
                "classify_tally: keep_confusion with C = %d above %d (the matrix alone would be over 128 MiB of state)", C,
                FRMAP_TALLY_MAX_CONFUSION_C);
  FRMAP_REQUIRE(logits && labels && state, "classify_tally: null pointer (logits, labels and state are required)");
  FRMAP_REQUIRE_ALIGNED(logits, 4, "logits");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(row_pred_out, 4, "row_pred_out");
  FRMAP_REQUIRE_ALIGNED(row_rank_out, 4, "row_rank_out");
  FRMAP_REQUIRE_ALIGNED(row_conf_out, 4, "row_conf_out");
  FRMAP_REQUIRE_ALIGNED(row_loss_out, 4, "row_loss_out");
  const int want = (B + TALLY_WAVES - 1) / TALLY_WAVES;
  const int blocks = want < TALLY_MAX_BLOCKS ? want : TALLY_MAX_BLOCKS;
  hipLaunchKernelGGL(classify_tally_kernel, dim3((unsigned)blocks), dim3(64 * TALLY_WAVES), 0, (hipStream_t)stream, logits, labels, B,
                     C, R, n_bins, keep_confusion, state, row_pred_out, row_rank_out, row_conf_out, row_loss_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_classify_tally_host(const float* logits_host, const int32_t* labels_host, int B, int C, int R, int n_bins,
                                         int keep_confusion, uint64_t* state_host, int32_t* row_pred_host, int32_t* row_rank_host,
                                         const float* row_conf_host, const float* row_loss_host) {
  const char* why = frmap_classify_tally_twin(logits_host, labels_host, B, C, R, n_bins, keep_confusion, state_host, row_pred_host,
                                              row_rank_host, row_conf_host, row_loss_host);
  FRMAP_REQUIRE(!why, "classify_tally_host: %s (B = %d, C = %d, R = %d, n_bins = %d, keep_confusion = %d)", why, B, C, R, n_bins,
                keep_confusion);
  return 0;
}
