// The grid arithmetic the head-fitting launchers share (head_fit.hip: the linear step and its groups; head_fit_hidden.hip).  Host
// code only: nothing here reaches a code object.
#pragma once
#include "head_fit_device.h"

// tiles of edge HF_T that cover n rows or columns of a GEMM operand
inline unsigned hf_tiles(int n) { return (unsigned)((n + HF_T - 1) / HF_T); }

// workgroups of the softmax kernel over B rows: a wavefront a row, HF_WAVES rows a workgroup, which loops beyond the cap
inline unsigned hf_softmax_blocks(int B) {
  const int want = (B + HF_WAVES - 1) / HF_WAVES;
  return (unsigned)(want < HF_SOFTMAX_MAX_BLOCKS ? want : HF_SOFTMAX_MAX_BLOCKS);
}
