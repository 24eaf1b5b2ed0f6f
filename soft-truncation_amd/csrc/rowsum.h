// rowsum.h -- the whole scaffold of a per-sample streaming kernel file (adaptive.hip, posterior.hip, guided.hip, edm.hip,
// consistency.hip, flow.hip, and sqloss.h between the last three): the size checks of their entries, the row grid, the layout of their
// [B, parts] workspaces of float64 partial sums, the device-side walk over that grid and the fixed-order float64 sums.
//
// The grid is two-dimensional because everything in those files is per sample: blockIdx.y walks the samples (striding when
// B exceeds the grid), blockIdx.x is one of the `parts` blocks that share a row and stride along it.  parts x rows is
// stk_ew_grid's cap of 8 blocks per CU at most, and parts depends on (B, n) alone -- not on the alignment -- so a workspace of
// partial sums has one layout, [B, parts, S] float64 (S sums per block; 1 everywhere but guided.hip's rescale), which a
// *_ws_bytes query can state without seeing a pointer.
//
// This header holds floating-point arithmetic: include it AFTER the file's `#pragma clang fp contract(off)` (stream.h:
// arithmetic belongs behind that pragma).  A kernel passes its bodies to the walks as lambdas; they are written in the
// including file, behind its pragma, like the rest of it.
#pragma once
#include "stream.h"

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

// 0, or the code every per-sample entry returns for B rows of `len` floats: everything fits 32-bit indices.
static inline int stk_row_check(int B, long len) {
  if (B <= 0 || len <= 0) return STK_EINVAL;
  if (len >= (1L << 31) || (long)B * len >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

// ... and every entry that streams over n elements without rows.
static inline int stk_length_check(long n) {
  if (n <= 0) return STK_EINVAL;
  if (n >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

// Bytes of the [B, parts(B, n), S] float64 workspace, and the test an entry makes of a plain (S = 1) one it is handed.
static inline long stk_row_ws_bytes(int B, long n, int S = 1) { return (long)B * stk_row_parts(B, n) * S * (long)sizeof(double); }
static inline bool stk_row_ws_ok(const void* ws, long ws_bytes, int B, long n) {
  return ws && (((uintptr_t)ws) & 7) == 0 && ws_bytes >= stk_row_ws_bytes(B, n);
}

static inline bool stk_positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }      // false for NaN and +inf

// How an entry launches on B rows of n floats: the 16-byte path when n is a multiple of 4 (an item never leaves its row) and
// every pointer given is 16-byte aligned (an absent optional one counts as aligned); `row` items of 4 or 1 elements per
// sample; the row grid, whose grid.x is the workspace's row length on either path.
struct StkRowPlan {
  bool vec;
  unsigned row;
  dim3 grid;
};
template <class... P>
static inline StkRowPlan stk_row_plan(int B, long n, const P*... p) {
  const bool vec = (n & 3) == 0 && stk_all_aligned16(p...);
  return {vec, (unsigned)(vec ? n >> 2 : n), dim3(stk_row_parts(B, n), stk_row_rows(B, n))};
}

// The walk of a kernel on the row grid: f(b) for the samples this block row visits, and inside it g(i) for the items of
// sample b this thread visits, i counted from the start of the tensor (b row + the item in the row; 32 bits, as the entries'
// checks allow).  The stride along a row is at most 2^19 items, so i + stride stays below 2^32.
template <class F>
__device__ __forceinline__ void row_samples(int B, F f) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) f(b);
}
template <class G>
__device__ __forceinline__ void row_items(unsigned row, int b, G g) {
  const unsigned stride = gridDim.x * 256;
  const unsigned base = (unsigned)b * row;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) g(base + i);
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

// This block's S sums over its stretch of row b, block-summed, into slot ((b parts + blockIdx.x) S + k) of the workspace.
template <int S>
__device__ __forceinline__ void row_store_partials(double (&acc)[S], double* red, double* ws, int b) {
#pragma unroll
  for (int k = 0; k < S; ++k) acc[k] = block_sum_f64(acc[k], red);
  if (threadIdx.x == 0) {
    double* slot = ws + ((size_t)b * gridDim.x + blockIdx.x) * S;
#pragma unroll
    for (int k = 0; k < S; ++k) slot[k] = acc[k];
  }
}
__device__ __forceinline__ void row_store_partial(double acc, double* red, double* ws, int b) {
  double a[1] = {acc};
  row_store_partials(a, red, ws, b);
}

// The S sums of row b from its `parts` partials: thread t adds partials t, t + 256, ... in index order, then the block sum.
// The same in every thread, and in every block that asks: no block reads what another block of its launch writes.
template <int S>
__device__ __forceinline__ void row_sum_partials(const double* ws, int b, unsigned parts, double* red, double (&s)[S]) {
#pragma unroll
  for (int k = 0; k < S; ++k) s[k] = 0.;
  for (unsigned j = threadIdx.x; j < parts; j += 256) {
    const double* slot = ws + ((size_t)b * parts + j) * S;
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] += slot[k];
  }
#pragma unroll
  for (int k = 0; k < S; ++k) s[k] = block_sum_f64(s[k], red);
}
__device__ __forceinline__ double row_sum_partial(const double* ws, int b, unsigned parts, double* red) {
  double s[1];
  row_sum_partials(ws, b, parts, red, s);
  return s[0];
}
