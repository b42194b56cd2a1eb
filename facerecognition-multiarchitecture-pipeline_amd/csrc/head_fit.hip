// One training step of a linear softmax head over cached trunk features (head_fit.LinearHead.step, head_fit.fit_head): softmax
// regression on a [B, D] view of a cached [N, D] matrix with an Adam / AdamW update, three launches and one small memset on the
// caller's stream, nothing copied to the host.  The rule, the summation order, the state and the workspace are head_fit_rule.h;
// head_fit.step_rule states the same in numpy and head_fit_twin.h on the host.
//
//   head_fit_logits_kernel   z = x' w^T + b.  A workgroup owns a 32 x 32 tile of z (32 batch rows x 32 classes) and all of its k.
//                            It also decides which of its rows are declined (row index, label, a non-finite feature - every
//                            feature passes through its staging loads) and, for the first class tile, writes row_src and adds the
//                            counted rows to n with one integer atomic.
//   head_fit_softmax_kernel  one wavefront per row: max, first arg-max, then in float64 the sum of exp, the row loss and
//                            g = (p - y) / n, each rounded to fp32 once; the figures reach the state as at most two integer
//                            atomics per workgroup.  n is complete here because the launch before wrote it.  Workgroup 0 advances
//                            t and adds n to `rows` when n > 0.
//   head_fit_update_kernel   dw = g^T x'.  A workgroup owns a 32 x 32 tile of w (32 classes x 32 features) and all of its k = B;
//                            each w[c][d] has one owner thread, which adds the chains, updates m and v and writes the weight.
//                            One more column of workgroups owns db and the bias the same way, against a column of ones.
// Both GEMMs cut k at multiples of FRMAP_HEAD_FIT_CHAIN = 128.  The four wavefronts of a workgroup take chains j, j + 1, j + 2,
// j + 3 of a round, each 64 steps of the fp32-input MFMA 32x32x2 (bit for bit fmaf over its two k, ascending) from +0, and leave
// their partial tiles in LDS; the owner threads then add them in ascending j.  A tile that the problem does not fill (a ragged
// edge: fewer than 32 rows or columns) runs the same chains as plain fmaf lanes over the same staged operands.  No float atomics,
// no dependency between workgroups inside a launch.
//
// frmap_head_fit_group_step runs H independent heads over one cache (head_fit_rule.h, GROUPS): one small kernel zeroes every head's n
// (and, with `clear`, its figures) - a kernel, not H strided memsets, so that a captured step holds one node for it -, then the same
// three kernel bodies with the head as blockIdx.z, each head reading its row of the device-resident hyper table where the single
// step takes scalars by value.  Head h gets the bits of the single step on its slices.  Flag 8 (evaluate only) stops after the
// softmax kernel, which then leaves t alone.
//
// LDS per workgroup: 4 x 2 x 32 x 33 floats of staging (pitch 33: the 32 lanes of an operand read 32 different banks) and
// 4 x 1024 floats of partial tiles = 50 176 bytes; the registers of the staging loads keep two workgroups a compute unit resident.
// The tile walk, the operand loaders and the three kernel bodies are head_fit_device.h, shared with head_fit_hidden.hip; so are the
// refusals (frmap_head_fit_refusal, head_fit_twin.h: the twins begin with the same list) and the grid arithmetic (head_fit_launch.h).
#include "head_fit_launch.h"

// (two wavefronts a SIMD: the 48 loads a lane keeps in flight cost registers, and a third resident workgroup would spill them)
__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_logits_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                        const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep,
                                                                        float keep_scale, const float* __restrict__ w,
                                                                        const float* __restrict__ b, uint64_t* state, float* __restrict__ z,
                                                                        int32_t* __restrict__ row_src, int N, int B, int D, int C) {
  hf_logits_body<false>(x, labels, rows, keep, keep_scale, w, b, state, z, row_src, nullptr, N, B, D, C, C);
}

// where head h of a group keeps its operands: H single-head operands each, the states `stride` bytes apart
struct HfGroup {
  size_t stride, work;       // bytes from one head's state / workspace to the next
  int B, D, C;
  __device__ __forceinline__ const int32_t* rows(const int32_t* p, int h) const { return p + (size_t)h * (size_t)B; }
  __device__ __forceinline__ const uint8_t* keep(const uint8_t* p, int h) const { return p ? p + (size_t)h * (size_t)B * (size_t)D : nullptr; }
  __device__ __forceinline__ float* w(float* p, int h) const { return p + (size_t)h * (size_t)C * (size_t)D; }
  __device__ __forceinline__ float* b(float* p, int h) const { return p + (size_t)h * (size_t)C; }
  __device__ __forceinline__ void* state(void* p, int h) const { return (char*)p + (size_t)h * stride; }
  __device__ __forceinline__ FrmapHeadFitWork workspace(void* p, int h) const { return frmap_head_fit_work((char*)p + (size_t)h * work, B, C); }
};

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_group_logits_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ labels, const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep,
    const float* __restrict__ hyper, float* w, float* b, void* state, void* workspace, HfGroup gr, int N) {
  const int h = blockIdx.z;
  const FrmapHeadFitWork wk = gr.workspace(workspace, h);
  hf_logits_body<false>(x, labels, gr.rows(rows, h), gr.keep(keep, h), hyper[(size_t)h * FRMAP_HEAD_FIT_HYPER_COLS + FRMAP_HEAD_FIT_HYPER_KEEP_SCALE],
                        gr.w(w, h), gr.b(b, h), (uint64_t*)gr.state(state, h), wk.z, wk.row_src, nullptr, N, gr.B, gr.D, gr.C, gr.C);
}


__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_softmax_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ row_src,
                                                                         uint64_t* state, const float* __restrict__ z, float* __restrict__ g,
                                                                         float* __restrict__ row_loss, int B, int C, float ls) {
  hf_softmax_body(labels, row_src, state, z, g, row_loss, B, C, ls, false);
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_group_softmax_kernel(const int32_t* __restrict__ labels, const float* __restrict__ hyper,
                                                                               void* state, void* workspace, HfGroup gr, int evaluate) {
  const int h = blockIdx.z;
  const FrmapHeadFitWork wk = gr.workspace(workspace, h);
  hf_softmax_body(labels, (const int32_t*)wk.row_src, (uint64_t*)gr.state(state, h), (const float*)wk.z, wk.g, wk.row_loss, gr.B, gr.C,
                  hyper[(size_t)h * FRMAP_HEAD_FIT_HYPER_COLS + 5], evaluate != 0);
}


__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                        float keep_scale, float* __restrict__ w, float* __restrict__ b,
                                                                        void* state, const float* __restrict__ g,
                                                                        const int32_t* __restrict__ row_src, int B, int D, int C,
                                                                        FrmapHeadFitHyper h, int flags) {
  hf_update_body(x, keep, keep_scale, w, b, state, g, row_src, B, D, C, h, flags);
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_group_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                              const float* __restrict__ hyper, float* w, float* b, void* state,
                                                                              void* workspace, HfGroup gr, int flags) {
  const int h = blockIdx.z;
  const float* r = hyper + (size_t)h * FRMAP_HEAD_FIT_HYPER_COLS;
  const FrmapHeadFitHyper hy = {r[0], r[1], r[2], r[3], r[4], r[5]};
  const FrmapHeadFitWork wk = gr.workspace(workspace, h);
  hf_update_body(x, gr.keep(keep, h), r[FRMAP_HEAD_FIT_HYPER_KEEP_SCALE], gr.w(w, h), gr.b(b, h), gr.state(state, h), (const float*)wk.g,
                 (const int32_t*)wk.row_src, gr.B, gr.D, gr.C, hy, flags);
}

// n of the step in flight of every head and, with `clear`, the three epoch figures behind it: one thread a head (a kernel, not H
// strided memset nodes, so that a captured step holds one node for it whatever H is)
__global__ __launch_bounds__(256) void head_fit_group_clear_kernel(void* state, size_t stride, int H, int clear) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  uint64_t* head = (uint64_t*)((char*)state + (size_t)h * stride);
  head[FRMAP_HEAD_FIT_N] = 0;
  if (clear) head[FRMAP_HEAD_FIT_ROWS] = head[FRMAP_HEAD_FIT_CORRECT] = head[FRMAP_HEAD_FIT_LOSS_Q] = 0;
}

extern "C" size_t frmap_head_fit_state_bytes(int D, int C, int amsgrad) {
  if (!frmap_head_fit_shape_ok(D, C)) return 0;
  return frmap_head_fit_state_size(D, C, amsgrad);
}

extern "C" size_t frmap_head_fit_workspace_bytes(int B, int D, int C) {
  if (!frmap_head_fit_shape_ok(D, C) || B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return 0;
  return frmap_head_fit_workspace_size(B, C);
}

extern "C" int frmap_head_fit_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale, float* w,
                                   float* b, void* state, void* workspace, int N, int B, int D, int C, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, float label_smoothing, int flags, void* stream) {
  const char* why = frmap_head_fit_linear_refusal(x, labels, w, b, state, workspace, N, B, D, C, flags, 7);
  FRMAP_REQUIRE(!why, "head_fit_step: %s (N = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, B, D, C, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(rows, 4, "rows");
  FRMAP_REQUIRE_ALIGNED(w, 4, "w");
  FRMAP_REQUIRE_ALIGNED(b, 4, "b");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const hipStream_t st = (hipStream_t)stream;
  uint64_t* head = (uint64_t*)state;
  const FrmapHeadFitWork wk = frmap_head_fit_work(workspace, B, C);
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  // n of the step in flight, and with `clear` the three epoch figures behind it (words 1 .. 4 of the header)
  if (hipMemsetAsync(head + FRMAP_HEAD_FIT_N, 0, (flags & FRMAP_HEAD_FIT_CLEAR) ? 32 : 8, st) != hipSuccess) {
    frmap_set_error("head_fit_step: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return -2;
  }
  const unsigned tb = hf_tiles(B), tc = hf_tiles(C), td = hf_tiles(D);
  hipLaunchKernelGGL(head_fit_logits_kernel, dim3(tc, tb), dim3(64 * HF_WAVES), 0, st, x, labels, rows, keep, keep_scale,
                     (const float*)w, (const float*)b, head, wk.z, wk.row_src, N, B, D, C);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_softmax_kernel, dim3(hf_softmax_blocks(B)), dim3(64 * HF_WAVES), 0, st, labels, (const int32_t*)wk.row_src, head,
                     (const float*)wk.z, wk.g, wk.row_loss, B, C, label_smoothing);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_update_kernel, dim3(td + 1, tc), dim3(64 * HF_WAVES), 0, st, x, keep, keep_scale, w, b, state,
                     (const float*)wk.g, (const int32_t*)wk.row_src, B, D, C, h, flags);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_head_fit_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                        float keep_scale, float* w_host, float* b_host, void* state_host, void* workspace_host, int N, int B,
                                        int D, int C, float lr, float beta1, float beta2, float eps, float weight_decay,
                                        float label_smoothing, int flags, int given_g) {
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  const char* why = frmap_head_fit_step_twin(x_host, labels_host, rows_host, keep_host, keep_scale, w_host, b_host, state_host,
                                             workspace_host, N, B, D, C, h, flags, given_g);
  FRMAP_REQUIRE(!why, "head_fit_step_host: %s (N = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, B, D, C, flags);
  return 0;
}

extern "C" size_t frmap_head_fit_group_state_stride(int D, int C, int amsgrad) {
  if (!frmap_head_fit_shape_ok(D, C)) return 0;
  return frmap_head_fit_group_stride(D, C, amsgrad);
}

extern "C" size_t frmap_head_fit_group_state_bytes(int H, int D, int C, int amsgrad) {
  if (!frmap_head_fit_shape_ok(D, C) || H < 1 || H > FRMAP_HEAD_FIT_MAX_H) return 0;
  return (size_t)H * frmap_head_fit_group_stride(D, C, amsgrad);
}

extern "C" size_t frmap_head_fit_group_workspace_bytes(int H, int B, int D, int C) {
  if (H < 1 || H > FRMAP_HEAD_FIT_MAX_H) return 0;
  return (size_t)H * frmap_head_fit_workspace_bytes(B, D, C);
}

extern "C" int frmap_head_fit_group_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, const float* hyper,
                                         float* w, float* b, void* state, void* workspace, int N, int H, int B, int D, int C, int flags,
                                         void* stream) {
  const char* why = frmap_head_fit_group_refusal(x, labels, rows, keep, hyper, w, b, state, workspace, N, H, B, D, C, flags);
  FRMAP_REQUIRE(!why, "head_fit_group_step: %s (N = %d, H = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, H, B, D, C, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(rows, 4, "rows");
  FRMAP_REQUIRE_ALIGNED(hyper, 4, "hyper");
  FRMAP_REQUIRE_ALIGNED(w, 4, "w");
  FRMAP_REQUIRE_ALIGNED(b, 4, "b");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const hipStream_t st = (hipStream_t)stream;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0, evaluate = (flags & FRMAP_HEAD_FIT_EVAL) ? 1 : 0;
  const HfGroup gr = {frmap_head_fit_group_stride(D, C, amsgrad), frmap_head_fit_workspace_size(B, C), B, D, C};
  hipLaunchKernelGGL(head_fit_group_clear_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, state, gr.stride, H,
                     (flags & FRMAP_HEAD_FIT_CLEAR) ? 1 : 0);
  FRMAP_LAUNCH_CHECK();
  // the grids of the single step, with the head as the slowest dimension (H <= 4096: within a grid's z)
  const unsigned tb = hf_tiles(B), tc = hf_tiles(C), td = hf_tiles(D);
  hipLaunchKernelGGL(head_fit_group_logits_kernel, dim3(tc, tb, (unsigned)H), dim3(64 * HF_WAVES), 0, st, x, labels, rows, keep, hyper, w, b, state,
                     workspace, gr, N);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_group_softmax_kernel, dim3(hf_softmax_blocks(B), 1u, (unsigned)H), dim3(64 * HF_WAVES), 0, st, labels, hyper, state,
                     workspace, gr, evaluate);
  FRMAP_LAUNCH_CHECK();
  if (evaluate) return 0;
  hipLaunchKernelGGL(head_fit_group_update_kernel, dim3(td + 1, tc, (unsigned)H), dim3(64 * HF_WAVES), 0, st, x, keep, hyper, w, b,
                     state, workspace, gr, flags);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_head_fit_group_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                              const float* hyper_host, float* w_host, float* b_host, void* state_host, void* workspace_host,
                                              int N, int H, int B, int D, int C, int flags, int given_g) {
  const char* why = frmap_head_fit_group_step_twin(x_host, labels_host, rows_host, keep_host, hyper_host, w_host, b_host, state_host,
                                                   workspace_host, N, H, B, D, C, flags, given_g);
  FRMAP_REQUIRE(!why, "head_fit_group_step_host: %s (N = %d, H = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, H, B, D, C, flags);
  return 0;
}
