// c4_grouped.hpp -- the one thing the grouped forms of the bf16 evaluator kernels add to the ungrouped ones
// (c4_conv_tower_bf16_grouped, c4_linear_bf16_grouped, c4_head_out_bf16_grouped): which model's weights a workgroup uses.
//
// The rows of a grouped batch are cut into one segment per model, seg_start[m] <= row < seg_start[m + 1], whose bounds live in
// device memory only (c4_session_route_leaves writes them) and are multiples of C4_GROUPED_ROW_ALIGN -- a multiple of every
// grouped kernel's rows per workgroup, so a workgroup never straddles two models.  The MoE "grouped GEMM" pattern: groups along
// the rows, sizes known on the device alone, one launch of a fixed shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c4grp {

struct Segments {
  const uint32_t* seg_start;   // [n_models + 1], ascending, seg_start[0] = 0
  uint32_t n_models;
  // The model whose segment holds `row` (the first row of a workgroup), -1 past the last segment.  Wavefront-uniform: scalar loads.
  // Always below n_models, whatever the array holds: a weight pointer never leaves the stacked operands.
  __device__ __forceinline__ int model_of(uint32_t row) const {
    int model = -1;
    for (uint32_t m = 0; m < n_models; m++)
      if (seg_start[m] <= row && row < seg_start[m + 1]) model = (int)m;
    return model;
  }
};

}  // namespace c4grp
