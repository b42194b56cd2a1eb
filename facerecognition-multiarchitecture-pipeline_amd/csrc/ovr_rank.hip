// Exact one-vs-rest ROC AUC and average precision without a sort: a class-major store of every score (frmap_ovr_append, one
// launch per batch) and, at the end, one count of pairs (frmap_ovr_rank_counts) that gives every counted row the three integers
// of ovr_rule.h; evaluate.ovr_metrics turns them into the per-class and macro figures of src/testing.py:296-312 and
// src/advanced_metrics.py:85-100 in float64 on the host.  The rule is ovr_rule.h; evaluate.ovr_rank_rule states it in numpy.
//
// Append: one launch, two kinds of work item on one grid (the branch is uniform in a workgroup).  A TILE item moves 64 rows x 64
// classes through LDS (pitch 65: the row-wise write and the column-wise read are both free of bank conflicts), so the read of
// scores[b][c] is contiguous in c and the write of store[c][first + b] contiguous in b.  A LABEL item gives four rows one wavefront
// each: lanes strided over the row, an integer test on the exponent bits, one ballot, and lane 0 stores the label of the rule.
//
// Count: a workgroup owns (class c, segment of rows j).  It walks the stored labels once, 1024 at a time (four loads in flight per
// thread), and compacts the positives of c into an LDS queue (ballot + popcount inside a wavefront, the four wavefront totals
// through LDS); whenever 256 are queued - and once more for the rest - every thread takes one positive, index and score in
// registers, and the workgroup streams its segment of column c and of the labels through LDS in chunks of 1024.  A row of the
// chunk is two floats: its score where it is of class c, and where it is of another class, NaN in the other field and in both
// for a declined row - NaN compares false both ways and so adds nothing, and the predicate of ovr_rule.h is called with a
// constant `same` (three compares and three adds a pair).  Every thread compares its positive against the chunk: all lanes read
// the same LDS address, a broadcast.  A batch of at most 64 positives is given to all four wavefronts, a quarter of the chunk
// each.  The three partial counts (32-bit: a segment is shorter than 2^31) go to the row's words as
// 64-bit integer atomic adds, zero amounts not issued; the words are zeroed by one small kernel ahead of the count in the same
// call.  A launch, not hipMemsetAsync: captured into a graph, the three memset nodes did not replay reliably - from the second or
// third replay on every word came back as a page-aligned address plus the right count, as if filled with a stale pattern - while a kernel node
// replays as it was launched (tests/test_stream_ops_gpu.py keeps the case).  Integer adds only: the words are the same bits on
// every run.  Every column is addressed as store + (size_t) c * capacity.
// Comparisons are fp32 compares with the default denormal mode (denormals kept); no flush-to-zero flag is given to this file.
#include "frmap_common.h"
#include "ovr_rule.h"
#include "ovr_twin.h"

constexpr int OVR_THREADS = 256;
constexpr int OVR_TILE = 64;                 // rows x classes of one transposed tile
constexpr int OVR_APPEND_MAX_BLOCKS = 8192;  // beyond that a workgroup takes several items
constexpr int OVR_CHUNK = 1024;              // rows of the segment in LDS at a time (8 KiB)
constexpr int OVR_WALK = 4;                  // labels a thread keeps in flight per step of the walk
constexpr int OVR_QUEUE = OVR_THREADS * (OVR_WALK + 1);   // fewer than 256 queued + at most 1024 new
constexpr int OVR_TARGET_BLOCKS = 2048;      // 8 per compute unit of 256: the segments per class are chosen to reach it

// one row of the chunk: its score in the column where the row is of the class / of another class, NaN in the other field
struct ovr_pair_t {
  float same;
  float other;
};

__global__ __launch_bounds__(OVR_THREADS) void ovr_append_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                 int B, int C, float* __restrict__ store,
                                                                 int32_t* __restrict__ store_labels, long long capacity, long long first,
                                                                 long long tiles_c, long long tiles, long long items) {
  __shared__ float tile[OVR_TILE][OVR_TILE + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    if (item < tiles) {                                    // (uniform in the workgroup)
      const long long b0 = (item / tiles_c) * OVR_TILE, c0 = (item % tiles_c) * OVR_TILE;
#pragma unroll
      for (int k = 0; k < OVR_TILE / 4; ++k) {
        const int bl = ty + 4 * k;
        const long long b = b0 + bl, c = c0 + tx;
        if (b < (long long)B && c < (long long)C) tile[bl][tx] = scores[(size_t)b * (size_t)C + (size_t)c];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < OVR_TILE / 4; ++k) {
        const int cl = ty + 4 * k;
        const long long c = c0 + cl, b = b0 + tx;
        if (c < (long long)C && b < (long long)B) store[(size_t)c * (size_t)capacity + (size_t)(first + b)] = tile[tx][cl];
      }
      __syncthreads();
    } else {
      const long long r = (item - tiles) * 4 + ty;         // (uniform in the wavefront)
      if (r < (long long)B) {
        const int32_t y = labels[r];
        bool bad = false;
        if (y >= 0 && y < C) {
          const float* z = scores + (size_t)r * (size_t)C;
          for (int c = tx; c < C; c += 64) bad |= !frmap_tally_finite_bits(__float_as_uint(z[c]));
        }
        const bool all_finite = __ballot(bad) == 0ull;
        if (tx == 0) store_labels[first + r] = frmap_ovr_stored_label(y, C, all_finite);
      }
    }
  }
}

__device__ __forceinline__ void ovr_add(uint64_t* p, unsigned v) {
  __hip_atomic_fetch_add((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(OVR_THREADS) void ovr_zero_kernel(uint64_t* __restrict__ ge_same, uint64_t* __restrict__ ge_other,
                                                               uint64_t* __restrict__ eq_other, long long n) {
  for (long long i = (long long)blockIdx.x * OVR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * OVR_THREADS) {
    ge_same[i] = 0;
    ge_other[i] = 0;
    eq_other[i] = 0;
  }
}

__global__ __launch_bounds__(OVR_THREADS) void ovr_rank_kernel(const float* __restrict__ store, const int32_t* __restrict__ store_labels,
                                                               int n, long long capacity, int C, int S, long long seg_len,
                                                               uint64_t* ge_same, uint64_t* ge_other, uint64_t* eq_other) {
  __shared__ ovr_pair_t s_pair[OVR_CHUNK];
  __shared__ int s_q[OVR_QUEUE];
  __shared__ int s_wtot[OVR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = (int)(blockIdx.x / (unsigned)S), seg = (int)(blockIdx.x % (unsigned)S);
  const long long j_lo = (long long)seg * seg_len;
  const long long j_hi = j_lo + seg_len < (long long)n ? j_lo + seg_len : (long long)n;
  if (j_lo >= j_hi) return;                                // (uniform)
  const float* col = store + (size_t)c * (size_t)capacity;

  // Entries [from, from + cnt) of the queue against the segment: one positive per thread - or, when one wavefront holds them all
  // (cnt <= 64), one per lane of EVERY wavefront, each wavefront taking its quarter of every chunk, so a class of few positives
  // still keeps four wavefronts busy (a row then receives four partial adds per word instead of one).
  auto process = [&](int from, int cnt) {
    const bool spread = cnt <= 64;                         // (uniform)
    const int slot = spread ? lane : tid;
    const bool mine = slot < cnt;
    const int idx = mine ? s_q[from + slot] : 0;
    const float s = mine ? col[idx] : 0.f;
    const int k_lo = spread ? wave * (OVR_CHUNK / 4) : 0;  // (uniform in the wavefront, and so is k_n)
    const int k_n = spread ? OVR_CHUNK / 4 : (wave * 64 < cnt ? OVR_CHUNK : 0);
    unsigned a = 0, b = 0, e = 0;
    for (long long j0 = j_lo; j0 < j_hi; j0 += OVR_CHUNK) {
#pragma unroll
      for (int k = 0; k < OVR_CHUNK / OVR_THREADS; ++k) {
        const int jj = tid + OVR_THREADS * k;
        const long long j = j0 + jj;
        ovr_pair_t p = {__builtin_nanf(""), __builtin_nanf("")};   // past the segment, or a declined row: adds nothing
        if (j < j_hi) {
          const int32_t lab = store_labels[j];
          if (frmap_ovr_counted(lab, C)) {
            const float v = col[j];
            if (lab == c) p.same = v;
            else p.other = v;
          }
        }
        s_pair[jj] = p;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < k_n; ++k) {
        const ovr_pair_t p = s_pair[k_lo + k];             // every lane the same address: a broadcast
        unsigned da, db, de, none;
        frmap_ovr_pair(p.same, s, true, &da, &none, &none);
        a += da;
        frmap_ovr_pair(p.other, s, false, &none, &db, &de);
        b += db;
        e += de;
      }
      __syncthreads();
    }
    if (mine) {
      if (a) ovr_add(ge_same + idx, a);
      if (b) ovr_add(ge_other + idx, b);
      if (e) ovr_add(eq_other + idx, e);
    }
  };

  int qn = 0;                                              // queued positives (the same number in every thread)
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long i0 = 0; i0 < (long long)n; i0 += OVR_THREADS * OVR_WALK) {
    int32_t lab[OVR_WALK];
#pragma unroll
    for (int k = 0; k < OVR_WALK; ++k) {                   // (OVR_WALK loads in flight; -1 is nobody's class)
      const long long i = i0 + k * OVR_THREADS + tid;
      lab[k] = i < (long long)n ? store_labels[i] : -1;
    }
    unsigned long long mask[OVR_WALK];
    int mine_total = 0;
#pragma unroll
    for (int k = 0; k < OVR_WALK; ++k) {
      mask[k] = __ballot(lab[k] == c);
      mine_total += __popcll(mask[k]);
    }
    if (lane == 0) s_wtot[wave] = mine_total;
    __syncthreads();
    int at = qn, total = 0;
#pragma unroll
    for (int w = 0; w < OVR_THREADS / 64; ++w) {
      const int t = s_wtot[w];
      at += w < wave ? t : 0;
      total += t;
    }
#pragma unroll
    for (int k = 0; k < OVR_WALK; ++k) {                   // (every slot is below qn + total <= 255 + 1024; their order is immaterial)
      if (lab[k] == c) s_q[at + __popcll(mask[k] & below)] = (int)(i0 + k * OVR_THREADS + tid);
      at += __popcll(mask[k]);
    }
    qn += total;
    __syncthreads();
    while (qn >= OVR_THREADS) {                            // (uniform) the last 256 of the queue: nothing has to move
      qn -= OVR_THREADS;
      process(qn, OVR_THREADS);
    }
  }
  if (qn > 0) process(0, qn);
}

extern "C" int frmap_ovr_append(const float* scores, const int32_t* labels, int B, int C, float* store, int32_t* store_labels,
                                long long capacity, long long first, void* stream) {
  FRMAP_REQUIRE(B >= 1, "ovr_append: B = %d is below 1", B);
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "ovr_append: B = %d rows exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  FRMAP_REQUIRE(C >= 1, "ovr_append: C = %d is below 1", C);
  FRMAP_REQUIRE(first >= 0, "ovr_append: first = %lld is negative", first);
  FRMAP_REQUIRE(capacity >= 0 && first <= capacity && (long long)B <= capacity - first,
                "ovr_append: first + B = %lld + %d exceeds capacity = %lld", first, B, capacity);
  FRMAP_REQUIRE(scores && labels && store && store_labels, "ovr_append: null pointer (scores, labels, store and store_labels are required)");
  FRMAP_REQUIRE_ALIGNED(scores, 4, "scores");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(store, 4, "store");
  FRMAP_REQUIRE_ALIGNED(store_labels, 4, "store_labels");
  const long long tiles_c = ((long long)C + OVR_TILE - 1) / OVR_TILE, tiles_b = ((long long)B + OVR_TILE - 1) / OVR_TILE;
  const long long tiles = tiles_c * tiles_b, items = tiles + ((long long)B + 3) / 4;
  const int blocks = items < OVR_APPEND_MAX_BLOCKS ? (int)items : OVR_APPEND_MAX_BLOCKS;
  hipLaunchKernelGGL(ovr_append_kernel, dim3((unsigned)blocks), dim3(OVR_THREADS), 0, (hipStream_t)stream, scores, labels, B, C, store,
                     store_labels, capacity, first, tiles_c, tiles, items);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_ovr_rank_counts(const float* store, const int32_t* store_labels, long long n, long long capacity, int C,
                                     uint64_t* ge_same_out, uint64_t* ge_other_out, uint64_t* eq_other_out, void* stream) {
  FRMAP_REQUIRE(n >= 1, "ovr_rank_counts: n = %lld is below 1", n);
  FRMAP_REQUIRE(n <= 0x7fffffffll, "ovr_rank_counts: n = %lld rows exceed 2^31 - 1", n);
  FRMAP_REQUIRE(n <= capacity, "ovr_rank_counts: n = %lld exceeds capacity = %lld", n, capacity);
  FRMAP_REQUIRE(C >= 1, "ovr_rank_counts: C = %d is below 1", C);
  FRMAP_REQUIRE(C <= FRMAP_GRID_WG256_MAX, "ovr_rank_counts: C = %d classes exceed the grid (at most %d)", C, FRMAP_GRID_WG256_MAX);
  FRMAP_REQUIRE(store && store_labels && ge_same_out && ge_other_out && eq_other_out,
                "ovr_rank_counts: null pointer (store, store_labels and the three outputs are required)");
  FRMAP_REQUIRE_ALIGNED(store, 4, "store");
  FRMAP_REQUIRE_ALIGNED(store_labels, 4, "store_labels");
  FRMAP_REQUIRE_ALIGNED(ge_same_out, 8, "ge_same_out");
  FRMAP_REQUIRE_ALIGNED(ge_other_out, 8, "ge_other_out");
  FRMAP_REQUIRE_ALIGNED(eq_other_out, 8, "eq_other_out");
  // segments per class: enough workgroups to fill the machine at few classes, never a segment below one chunk
  const long long chunks = (n + OVR_CHUNK - 1) / OVR_CHUNK;
  long long S = (OVR_TARGET_BLOCKS + C - 1) / C;
  if (S > chunks) S = chunks;
  const long long seg_len = ((chunks + S - 1) / S) * OVR_CHUNK;
  S = (n + seg_len - 1) / seg_len;                         // (no empty segment)
  const long long zero_blocks = (n + OVR_THREADS - 1) / OVR_THREADS;
  hipLaunchKernelGGL(ovr_zero_kernel, dim3((unsigned)(zero_blocks < OVR_TARGET_BLOCKS ? zero_blocks : OVR_TARGET_BLOCKS)), dim3(OVR_THREADS), 0,
                     (hipStream_t)stream, ge_same_out, ge_other_out, eq_other_out, n);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ovr_rank_kernel, dim3((unsigned)((long long)C * S)), dim3(OVR_THREADS), 0, (hipStream_t)stream, store, store_labels,
                     (int)n, capacity, C, (int)S, seg_len, ge_same_out, ge_other_out, eq_other_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_ovr_rank_counts_host(const float* store_host, const int32_t* store_labels_host, long long n, long long capacity,
                                          int C, uint64_t* ge_same_host, uint64_t* ge_other_host, uint64_t* eq_other_host) {
  const char* why = frmap_ovr_rank_counts_twin(store_host, store_labels_host, n, capacity, C, ge_same_host, ge_other_host, eq_other_host);
  FRMAP_REQUIRE(!why, "ovr_rank_counts_host: %s (n = %lld, capacity = %lld, C = %d)", why, n, capacity, C);
  return 0;
}
