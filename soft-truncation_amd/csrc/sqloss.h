// sqloss.h -- the squared-residual loss that edm.hip, consistency.hip and flow.hip share: one loss kernel, one finishing kernel and
// one gradient kernel on the scaffold of rowsum.h, and the two launch sequences of their entries.  The files that include
// it give the expressions: how r is formed, what the row's sum becomes, where the gradient's factor comes from.
//
//   loss:    r = Res(operands);  q = r r;  acc += (double)q;  r kept when asked;  the block's partial to ws[b, blockIdx.x]
//   finish:  the row's partials in index order within the fixed tree, then Fin(acc, b) on one thread
//   grad:    dF = k[b] r,  k[b] = K(b)
//
// This header holds floating-point arithmetic: include it AFTER the file's `#pragma clang fp contract(off)`.
#pragma once
#include "rowsum.h"

// Res: `in[N]`, the N operand tensors in load order;  `row(b, B)` loads the coefficients of sample b;  `r(c, x)` is the
// residual of one element from those coefficients and its N operands.  row: items of V elements per sample.
template <int V, class Res>
__global__ __launch_bounds__(256) void sq_loss_kernel(unsigned row, int B, Res res, float* r_out, double* ws) {
  __shared__ double red[4];
  row_samples(B, [&](int b) {
    const auto c = res.row(b, B);
    double acc = 0.;
    row_items(row, b, [&](unsigned i) {
      Vec<V> in[Res::N], o;
#pragma unroll
      for (int k = 0; k < Res::N; ++k) in[k] = Vec<V>::load(res.in[k], i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float x[Res::N];
#pragma unroll
        for (int k = 0; k < Res::N; ++k) x[k] = in[k].v[j];
        const float r = Res::r(c, x);
        const float q = r * r;
        acc += (double)q;
        o.v[j] = r;
      }
      if (r_out) o.store(r_out, i);
    });
    row_store_partial(acc, red, ws, b);
  });
}

// One block per sample (striding).  Fin: `fin(acc, b, B)` turns the row's sum into the outputs, float64, each rounded once.
template <class Fin>
__global__ __launch_bounds__(256) void sq_loss_finish_kernel(const double* ws, int B, int parts, Fin fin) {
  __shared__ double red[4];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const double acc = row_sum_partial(ws, b, parts, red);
    if (threadIdx.x == 0) fin(acc, b, B);
  }
}

// K: `k(b, B)` is the factor of sample b, fp32.
template <int V, class K>
__global__ __launch_bounds__(256) void sq_loss_grad_kernel(unsigned row, int B, K k, const float* r, float* dF) {
  row_samples(B, [&](int b) {
    const float kb = k(b, B);
    row_items(row, b, [&](unsigned i) {
      const auto rv = Vec<V>::load(r, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = kb * rv.v[j];
      o.store(dF, i);
    });
  });
}

// The loss entry's two launches, after its checks; p = stk_row_plan of the operands and r_out.
template <class Res, class Fin>
static inline int sq_loss_launch(const StkRowPlan& p, int B, Res res, Fin fin, float* r_out, void* ws, hipStream_t stream) {
  const int launched = stk_launch_vec(p.vec, sq_loss_kernel<4, Res>, sq_loss_kernel<1, Res>, p.grid, stream, p.row, B, res, r_out,
                                      (double*)ws);
  if (launched != STK_OK) return launched;
  hipLaunchKernelGGL(sq_loss_finish_kernel<Fin>, dim3(B < STK_MAX_GRID ? B : STK_MAX_GRID), dim3(256), 0, stream,
                     (const double*)ws, B, (int)p.grid.x, fin);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

// ... and the gradient entry's one.
template <class K>
static inline int sq_loss_grad_launch(int B, long inner, K k, const float* r, float* dF, hipStream_t stream) {
  const StkRowPlan p = stk_row_plan(B, inner, r, dF);
  return stk_launch_vec(p.vec, sq_loss_grad_kernel<4, K>, sq_loss_grad_kernel<1, K>, p.grid, stream, p.row, B, k, r, dF);
}
