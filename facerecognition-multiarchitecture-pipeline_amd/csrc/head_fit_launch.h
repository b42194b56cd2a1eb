// The grid arithmetic the head-fitting launchers share (head_fit.hip: the linear step and its groups; head_fit_hidden.hip;
// head_fit_pair.hip; head_fit_margin.hip; head_fit_embed.hip) and the two halves of the margin launcher.  Host code only: nothing here
// reaches a code object.
#pragma once
#include "head_fit_device.h"

// tiles of edge HF_T that cover n rows or columns of a GEMM operand
inline unsigned hf_tiles(int n) { return (unsigned)((n + HF_T - 1) / HF_T); }

// workgroups of the softmax kernel over B rows: a wavefront a row, HF_WAVES rows a workgroup, which loops beyond the cap
inline unsigned hf_softmax_blocks(int B) {
  const int want = (B + HF_WAVES - 1) / HF_WAVES;
  return (unsigned)(want < HF_SOFTMAX_MAX_BLOCKS ? want : HF_SOFTMAX_MAX_BLOCKS);
}

// The two halves of the margin step's launcher (head_fit_margin.hip), which frmap_head_fit_margin_step runs back to back on its own
// operands and the embedding step (head_fit_embed.hip) around its own kernels.  Not exported; nothing is checked here.
//   forward: the memset of n of `head` (with bit 4 of `flags`: of the three figure words behind it), then the logits, norms and
//            softmax kernels - z, rx, rw, cosv, g, h, row_loss and row_src of `workspace`; n, the figures and t += 1 in `head`, the
//            8-word header of a margin state or 8 words that stand in for it.  Bit 16 of `flags` is the easy margin.  `who` names
//            the entry point in an error text.
//   update : the update kernel on (x, keep, g, h, rw, row_src) of `workspace`: it reads t and n from the header of `state`.
int frmap_head_fit_margin_forward_launch(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                         const float* w, uint64_t* head, void* workspace, int N, int B, int D, int C, float s, float m,
                                         float label_smoothing, int flags, hipStream_t st, const char* who);
int frmap_head_fit_margin_update_launch(const float* x, const uint8_t* keep, float keep_scale, float* w, void* state, void* workspace, int B,
                                        int D, int C, const FrmapHeadFitHyper& h, int flags, hipStream_t st);
