// One training step of a head with one hidden layer, Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C), over cached trunk features
// (head_fit.HiddenHead.step, head_fit.fit_head(hidden=...)): the rule, the state and the workspace are head_fit_rule.h, HIDDEN LAYER;
// head_fit.hidden_step_rule states the same in numpy and head_fit_twin.h on the host.  One small memset and six launches on the
// caller's stream, nothing copied to the host:
//   the memset of layer 2's n (with `clear`: its figures), as the linear step does it;
//   head_fit_hidden_forward_kernel  h = relu(x' w1^T + b1): the logits tile walk (hf_logits_body) with the ReLU epilogue.  It decides
//                                   layer 1's declined rows as that body does, writes h, lab and row_src1, and counts nothing.
//   head_fit_hidden_logits_kernel, head_fit_hidden_softmax_kernel
//                                   the linear step's two forward bodies on (h, lab, NULL, keep2, w2, b2, state 2).
//   head_fit_hidden_back_kernel     da = gate (g w2): a workgroup per 32 x 32 tile of da over all k = C; A = g with k contiguous,
//                                   B = w2 with k the slow axis (one layout flag per operand of hf_tile_chains).  One thread copies
//                                   t and n of state 2 into state 1.
//   head_fit_hidden_update_kernel   the linear step's update body, on layer 2 with (h, keep2, g, row_src2), then on layer 1 with
//                                   g := da and C := Hd on (x, keep1, row_src1).
// The launch after the back kernel is the only ordering constraint - w2 must not change before da is written - and the stream order
// gives it.  No grid barrier, no flags between workgroups, no float atomics; integer atomics only where the shared bodies have them.
// The three wrappers around the shared bodies are this file's own kernels: the bits are the linear step's (tests/
// test_head_fit_hidden_gpu.py compares them kernel against kernel), and head_fit.hip's code object does not change with this file.
#include "head_fit_launch.h"

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_hidden_logits_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ labels, const uint8_t* __restrict__ keep, float keep_scale, const float* __restrict__ w,
    const float* __restrict__ b, uint64_t* state, float* __restrict__ z, int32_t* __restrict__ row_src, int B, int D, int C) {
  hf_logits_body<false>(x, labels, nullptr, keep, keep_scale, w, b, state, z, row_src, nullptr, B, B, D, C, C);
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_hidden_softmax_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ row_src,
                                                                                uint64_t* state, const float* __restrict__ z, float* __restrict__ g,
                                                                                float* __restrict__ row_loss, int B, int C, float ls) {
  hf_softmax_body(labels, row_src, state, z, g, row_loss, B, C, ls, false);
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_hidden_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                               float keep_scale, float* __restrict__ w, float* __restrict__ b,
                                                                               void* state, const float* __restrict__ g,
                                                                               const int32_t* __restrict__ row_src, int B, int D, int C,
                                                                               FrmapHeadFitHyper h, int flags) {
  hf_update_body(x, keep, keep_scale, w, b, state, g, row_src, B, D, C, h, flags);
}

// Layer 1 forward: the logits tile walk over w1 with the ReLU epilogue; writes h, lab and row_src1 and counts nothing.
__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_hidden_forward_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ labels, const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep1,
    float keep1_scale, const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ h, int32_t* __restrict__ row_src1,
    int32_t* __restrict__ lab, int N, int B, int D, int Hd, int C) {
  hf_logits_body<true>(x, labels, rows, keep1, keep1_scale, w1, b1, nullptr, h, row_src1, lab, N, B, D, Hd, C);
}

// the operands of the back tile (b0, j0) of da, k = the class: A = g of the batch rows (k is contiguous in g), B = w2, whose k is the
// slow axis (consecutive lanes walk the hidden units of one class, which are contiguous in w2)
struct HfBackOp {
  const float* g;
  const float* w2;
  int b0, j0, B, Hd, C;
  __device__ __forceinline__ void load(int k0, int K, int li, int lk, float (&a)[16], float (&b)[16]) const {
    float gv[16], wv[16];
    const int ka = k0 + li;
    const size_t kac = (size_t)(ka < K ? ka : K - 1), ji = (size_t)(j0 + li < Hd ? j0 + li : Hd - 1);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int bi = b0 + it * 2 + lk;
      gv[it] = g[(size_t)(bi < B ? bi : B - 1) * (size_t)C + kac];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int k = k0 + it * 2 + lk;
      wv[it] = w2[(size_t)(k < K ? k : K - 1) * (size_t)Hd + ji];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      a[it] = (ka < K && b0 + it * 2 + lk < B) ? gv[it] : 0.0f;
      b[it] = (k0 + it * 2 + lk < K && j0 + li < Hd) ? wv[it] : 0.0f;
    }
  }
};

// Back: da = relu'(h) mask2 (g w2).  A workgroup owns a 32 x 32 tile of da (32 batch rows x 32 hidden units) and all of its k = C.  It
// reads w2, so it runs before layer 2's update; the stream order gives that.  One thread copies t and n of layer 2's state (the softmax
// kernel has advanced t) into layer 1's, where layer 1's update kernel reads them.
__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_hidden_back_kernel(
    const float* __restrict__ g, const float* __restrict__ w2, const float* __restrict__ h, const uint8_t* __restrict__ keep2, float keep2_scale,
    const int32_t* __restrict__ row_src2, float* __restrict__ da, uint64_t* state1, const uint64_t* state2, int B, int Hd, int C) {
  __shared__ HfSmem sm;
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * HF_T, b0 = blockIdx.y * HF_T;
  const int vi = B - b0 < HF_T ? B - b0 : HF_T, vj = Hd - j0 < HF_T ? Hd - j0 : HF_T;
  float tot[4];
  const HfBackOp op = {g, w2, b0, j0, B, Hd, C};
  hf_tile_chains<true, false>(sm, C, vi < HF_T || vj < HF_T, vi, vj, op, tot);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = b0 + (tid >> 5) + 8 * q, j = j0 + (tid & 31);
    if (i < B && j < Hd) {
      const size_t at = (size_t)i * (size_t)Hd + j;
      da[at] = frmap_head_fit_da(tot[q], h[at], keep2 ? (int)keep2[at] : -1, keep2_scale, row_src2[i] >= 0);
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    state1[FRMAP_HEAD_FIT_T] = state2[FRMAP_HEAD_FIT_T];
    state1[FRMAP_HEAD_FIT_N] = state2[FRMAP_HEAD_FIT_N];
  }
}

extern "C" size_t frmap_head_fit_hidden_state_bytes(int D, int Hd, int C, int amsgrad) {
  if (!frmap_head_fit_hidden_shape_ok(D, Hd, C)) return 0;
  return frmap_head_fit_hidden_state_size(D, Hd, C, amsgrad);
}

extern "C" size_t frmap_head_fit_hidden_workspace_bytes(int B, int D, int Hd, int C) {
  if (!frmap_head_fit_hidden_shape_ok(D, Hd, C) || B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return 0;
  return frmap_head_fit_hidden_workspace_size(B, Hd, C);
}

extern "C" int frmap_head_fit_hidden_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep1, float keep1_scale,
                                          const uint8_t* keep2, float keep2_scale, float* w1, float* b1, float* w2, float* b2, void* state,
                                          void* workspace, int N, int B, int D, int Hd, int C, float lr, float beta1, float beta2, float eps,
                                          float weight_decay, float label_smoothing, int flags, void* stream) {
  const char* why = frmap_head_fit_hidden_refusal(x, labels, w1, b1, w2, b2, state, workspace, N, B, D, Hd, C, flags);
  FRMAP_REQUIRE(!why, "head_fit_hidden_step: %s (N = %d, B = %d, D = %d, Hd = %d, C = %d, flags = %d)", why, N, B, D, Hd, C, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(rows, 4, "rows");
  FRMAP_REQUIRE_ALIGNED(w1, 4, "w1");
  FRMAP_REQUIRE_ALIGNED(b1, 4, "b1");
  FRMAP_REQUIRE_ALIGNED(w2, 4, "w2");
  FRMAP_REQUIRE_ALIGNED(b2, 4, "b2");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const hipStream_t st = (hipStream_t)stream;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  void* state2 = (char*)state + frmap_head_fit_state_size(D, Hd, amsgrad);
  uint64_t* head1 = (uint64_t*)state;
  uint64_t* head2 = (uint64_t*)state2;
  const FrmapHeadFitHiddenWork wk = frmap_head_fit_hidden_work(workspace, B, Hd);
  const FrmapHeadFitWork wk2 = frmap_head_fit_work(wk.layer2, B, C);
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  // n of the step in flight of layer 2, and with `clear` its three epoch figures, as the single step does it
  if (hipMemsetAsync(head2 + FRMAP_HEAD_FIT_N, 0, (flags & FRMAP_HEAD_FIT_CLEAR) ? 32 : 8, st) != hipSuccess) {
    frmap_set_error("head_fit_hidden_step: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return -2;
  }
  const unsigned tb = hf_tiles(B), tc = hf_tiles(C), td = hf_tiles(D), th = hf_tiles(Hd);
  const dim3 block(64 * HF_WAVES);
  hipLaunchKernelGGL(head_fit_hidden_forward_kernel, dim3(th, tb), block, 0, st, x, labels, rows, keep1, keep1_scale,
                     (const float*)w1, (const float*)b1, wk.h, wk.row_src1, wk.lab, N, B, D, Hd, C);
  FRMAP_LAUNCH_CHECK();
  // layer 2 forward: the single step's two kernels on (h, lab), N = B, rows = NULL
  hipLaunchKernelGGL(head_fit_hidden_logits_kernel, dim3(tc, tb), block, 0, st, (const float*)wk.h, (const int32_t*)wk.lab,
                     keep2, keep2_scale, (const float*)w2, (const float*)b2, head2, wk2.z, wk2.row_src, B, Hd, C);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_hidden_softmax_kernel, dim3(hf_softmax_blocks(B)), block, 0, st,
                     (const int32_t*)wk.lab, (const int32_t*)wk2.row_src, head2, (const float*)wk2.z, wk2.g, wk2.row_loss, B, C, label_smoothing);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_hidden_back_kernel, dim3(th, tb), block, 0, st, (const float*)wk2.g, (const float*)w2,
                     (const float*)wk.h, keep2, keep2_scale, (const int32_t*)wk2.row_src, wk.da, head1, (const uint64_t*)head2, B, Hd, C);
  FRMAP_LAUNCH_CHECK();
  // w2 changes only now, after da was written from it
  hipLaunchKernelGGL(head_fit_hidden_update_kernel, dim3(th + 1, tc), block, 0, st, (const float*)wk.h, keep2, keep2_scale, w2, b2,
                     state2, (const float*)wk2.g, (const int32_t*)wk2.row_src, B, Hd, C, h, flags);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_hidden_update_kernel, dim3(td + 1, th), block, 0, st, x, keep1, keep1_scale, w1, b1, state,
                     (const float*)wk.da, (const int32_t*)wk.row_src1, B, D, Hd, h, flags);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_head_fit_hidden_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep1_host,
                                               float keep1_scale, const uint8_t* keep2_host, float keep2_scale, float* w1_host, float* b1_host,
                                               float* w2_host, float* b2_host, void* state_host, void* workspace_host, int N, int B, int D,
                                               int Hd, int C, float lr, float beta1, float beta2, float eps, float weight_decay,
                                               float label_smoothing, int flags, int given_g) {
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  const char* why = frmap_head_fit_hidden_step_twin(x_host, labels_host, rows_host, keep1_host, keep1_scale, keep2_host, keep2_scale, w1_host,
                                                    b1_host, w2_host, b2_host, state_host, workspace_host, N, B, D, Hd, C, h, flags, given_g);
  FRMAP_REQUIRE(!why, "head_fit_hidden_step_host: %s (N = %d, B = %d, D = %d, Hd = %d, C = %d, flags = %d)", why, N, B, D, Hd, C, flags);
  return 0;
}
