// flow.hip -- the element-wise launches of rectified flow (include/stk_flow.h, gfx950): the velocity loss and its gradient,
// and the one step launch of the sampler in its Euler, correction and stochastic forms.
//
// Everything streams once over the [B, inner] batch or the n-element state -- loss reads 3 and writes 1 tensor (12 + 4 B per
// element), loss_grad reads 1 and writes 1 (4 + 4 B), the Euler step reads 2 and writes 1 (12 B), the correction and the
// stochastic step read 3 and write 1 (16 B): HBM-bound, and laid out as stream.h describes, the 16-byte path taken whenever
// the row length (or n) is a multiple of 4.  The per-sample launches use the row grid of rowsum.h; the workspace of the
// loss's partial sums is its [B, parts(B, inner)] float64 layout, which stk_flow_ws_bytes states without seeing a pointer.
// B inner < 2^31 and n < 2^31 (checked by the entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
// stream.h, included before it, holds loads, stores and host code only; rowsum.h and sqloss.h (the loss, finish and gradient
// kernels shared with edm.hip and consistency.hip) hold arithmetic and follow the pragma.
#include "stream.h"
#include "stk_flow.h"

#pragma clang fp contract(off)

#include "rowsum.h"
#include "sqloss.h"

namespace {

// r = F - (n - y), both differences rounded to fp32 in that order.  No per-sample coefficient.
struct FlowRes {
  static constexpr int N = 3;
  const float* in[N];                                      // F, y, n
  struct Row {};
  __device__ Row row(int, int) const { return {}; }
  __device__ static float r(const Row&, const float* v) {
    const float u = v[2] - v[1];
    return v[0] - u;
  }
};

// The row's sum, rounded once.
struct FlowFinish {
  float* loss;
  double inner;
  int reduce_mean;
  __device__ void operator()(double acc, int b, int) const { loss[b] = (float)(reduce_mean ? acc / inner : acc); }
};

struct FlowGradFactor {
  const float* dloss;
  float inner;
  int reduce_mean;
  __device__ float operator()(int b, int) const {
    float k = 2.f * dloss[b];
    if (reduce_mean) k = k / inner;
    return k;
  }
};

struct StepArgs {
  const float* xb; const float* v; const float* v_prev; const float* eps;
  float* x_out;
  float cx, cv, cn;
};

// total: items of V elements.  The stride is at most 2^19 items, so i + stride stays below 2^32.
template <int V>
__global__ __launch_bounds__(256) void flow_step_kernel(unsigned total, StepArgs a) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto bv = Vec<V>::load(a.xb, i);
    const auto vv = Vec<V>::load(a.v, i);
    Vec<V> pv, ev, xo;
    if (a.v_prev) pv = Vec<V>::load(a.v_prev, i);
    if (a.eps) ev = Vec<V>::load(a.eps, i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float slope = a.v_prev ? 0.5f * pv.v[j] + 0.5f * vv.v[j] : vv.v[j];
      const float m = a.cx * bv.v[j];
      const float p = a.cv * slope;
      float x = m + p;
      if (a.eps) x = x + a.cn * ev.v[j];
      xo.v[j] = x;
    }
    xo.store(a.x_out, i);
  }
}

}  // namespace

extern "C" long stk_flow_ws_bytes(int B, long inner) {
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return stk_row_ws_bytes(B, inner);
}

extern "C" int stk_flow_loss_f32(const float* F, const float* y, const float* n, void* ws, long ws_bytes, float* r_out,
                                 float* loss_out, int B, long inner, int reduce_mean, void* stream) {
  if (!F || !y || !n || !ws || !loss_out) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, B, inner)) return STK_EINVAL;
  return sq_loss_launch(stk_row_plan(B, inner, F, y, n, r_out), B, FlowRes{{F, y, n}},
                        FlowFinish{loss_out, (double)inner, reduce_mean}, r_out, ws, (hipStream_t)stream);
}

extern "C" int stk_flow_loss_grad_f32(const float* r, const float* dloss, float* dF, int B, long inner, int reduce_mean,
                                      void* stream) {
  if (!r || !dloss || !dF) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return sq_loss_grad_launch(B, inner, FlowGradFactor{dloss, (float)inner, reduce_mean}, r, dF, (hipStream_t)stream);
}

extern "C" int stk_flow_step_f32(const float* xb, const float* v, const float* v_prev, const float* eps, float cx, float cv,
                                 float cn, float* x_out, long n, void* stream) {
  if (!xb || !v || !x_out || !(cn >= 0.f)) return STK_EINVAL;
  if ((v_prev && eps) || (!eps && cn != 0.f)) return STK_EINVAL;
  const int rc = stk_length_check(n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(xb, v, v_prev, eps, x_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  StepArgs a{xb, v, v_prev, eps, x_out, cx, cv, cn};
  return stk_launch_vec(vec, flow_step_kernel<4>, flow_step_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}
