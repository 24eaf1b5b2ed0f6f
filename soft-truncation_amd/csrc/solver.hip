// solver.hip -- the update of the DPM-Solver++ samplers (include/stk_solver.h, gfx950).
//
// One streaming pass per network evaluation: it reads x, the score and (second order) the previous data prediction and
// writes x and the data prediction, at most 12 B read and 8 B written per element, around seven multiply-adds -- HBM-bound,
// and laid out as stream.h describes, the 16-byte path taken whenever n is a multiple of 4.  n < 2^31 (checked by the
// entry), so the index arithmetic is 32-bit.
// The five coefficients and the two bounds are launch arguments: nothing is read from a table.
#include "stream.h"
#include "stk_solver.h"

namespace {

// The operands of one launch.  x_out may be x and d_out may be d_prev: an item reads all it needs before it writes, and no
// two items share an element.
struct Args {
  const float* x; const float* score; const float* d_prev;
  float* x_out; float* d_out;
  float cx, cs, g, A, B, lo, hi;
};

// total: items of V elements.  The stride is at most 2^19 items, so i + stride stays below 2^32.
template <int V>
__global__ __launch_bounds__(256) void dpm_update_kernel(unsigned total, Args a) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto xv = Vec<V>::load(a.x, i);
    const auto sv = Vec<V>::load(a.score, i);
    Vec<V> pv;
    if (a.d_prev) pv = Vec<V>::load(a.d_prev, i);
    Vec<V> xo, dv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float d = a.cx * xv.v[j] + a.cs * sv.v[j];
      d = fminf(fmaxf(d, a.lo), a.hi);
      const float D = a.d_prev ? d + a.g * (d - pv.v[j]) : d;
      xo.v[j] = a.A * xv.v[j] + a.B * D;
      dv.v[j] = d;
    }
    xo.store(a.x_out, i);
    if (a.d_out) dv.store(a.d_out, i);
  }
}

}  // namespace

extern "C" int stk_dpm_update_f32(const float* x, const float* score, const float* d_prev, float cx, float cs, float g, float A,
                                  float B, float clip_lo, float clip_hi, float* x_out, float* d_out, long n, void* stream) {
  if (!x || !score || !x_out || n <= 0 || (g != 0.f && !d_prev) || !(clip_lo <= clip_hi)) return STK_EINVAL;
  if (n >= (1L << 31)) return STK_EUNSUPPORTED;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, score, x_out, d_prev, d_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  Args a{x, score, d_prev, x_out, d_out, cx, cs, g, A, B, clip_lo, clip_hi};
  return stk_launch_vec(vec, dpm_update_kernel<4>, dpm_update_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}
