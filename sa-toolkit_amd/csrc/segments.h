// The table lookups of the segment kernels on a packed time axis (include/satools_hip_ragged.h, satools_hip_ragged2d.h), with their range
// checks: shared by csrc/ragged/, csrc/ragged2d/ and csrc/ragged2d16/.
#pragma once

namespace sat {

// segment i of one table -> (first column, columns); false for an entry that does not lie inside 0 .. T - 1
__device__ __forceinline__ bool ragged_segment(const int* __restrict__ seg_off, const int* __restrict__ seg_len, int i, int T, int* off, int* len) {
  const int o = seg_off[i], l = seg_len[i];
  *off = o;
  *len = l;
  return o >= 0 && l >= 1 && o < T && l <= T - o;
}

// segment i of a conv: W input columns from column `in` of x's rows, Wo = (W - 1) / S + 1 output columns from column `out` of y's rows;
// false unless both lie inside their rows and W <= max_len (the bound the grid was sized by: a longer segment would be computed in part)
__device__ __forceinline__ bool ragged_conv_segment(const int* __restrict__ in_off, const int* __restrict__ in_len, const int* __restrict__ out_off, int i,
                                             int T_in, int T_out, int max_len, int S, int* in, int* W, int* out, int* Wo) {
  if (!ragged_segment(in_off, in_len, i, T_in, in, W) || *W > max_len) return false;
  const int o = out_off[i], wo = (*W - 1) / S + 1;
  *out = o;
  *Wo = wo;
  return o >= 0 && o < T_out && wo <= T_out - o;
}

}  // namespace sat
