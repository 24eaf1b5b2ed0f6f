// rowsum.h -- what the per-sample streaming kernels share (adaptive.hip, posterior.hip): the row grid and the fixed-order
// float64 block sum behind their [B, parts] workspaces of partial sums.
//
// The grid is two-dimensional because everything in those files is per sample: blockIdx.y walks the samples (striding when
// B exceeds the grid), blockIdx.x is one of the `parts` blocks that share a row and stride along it.  parts x rows is
// stk_ew_grid's cap of 8 blocks per CU at most, and parts depends on (B, n) alone -- not on the alignment -- so a workspace of
// partial sums has one layout, [B, parts] float64, which a *_ws_bytes query can state without seeing a pointer.
//
// Include it AFTER the file's `#pragma clang fp contract(off)` (stream.h: arithmetic belongs behind that pragma).
#pragma once
#include "common.h"

// Rows walked at once, and blocks that share one row: functions of (B, n) alone.
static inline int stk_row_rows(int B, long n) {
  const int g = stk_ew_grid((long)B * n);
  return B < g ? B : g;
}
static inline int stk_row_parts(int B, long n) {
  long p = stk_ew_grid((long)B * n) / stk_row_rows(B, n);
  const long blocks_per_row = (n + 255) / 256;
  if (p > blocks_per_row) p = blocks_per_row;
  return (int)(p < 1 ? 1 : p);
}

// Block-wide float64 sum in a fixed order: xor butterfly inside each wave, then the four waves in index order.  The result
// is the same in every thread.  Ends with a barrier so `red` (4 doubles) can be reused.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}
