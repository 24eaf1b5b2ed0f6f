// edm.hip -- the element-wise launches of the EDM formulation (include/stk_edm.h, gfx950): the per-sample coefficients, the
// weighted denoising loss and its gradient, and the churn / Heun launches of the sampler.
//
// Everything but the coefficients streams once over the [B, inner] batch or the n-element state -- loss reads 3 and writes 1
// tensor (12 + 4 B per element), loss_grad reads 1 and writes 1 (4 + 4 B), churn reads 1-2 and writes 2, the Euler stage reads
// 2 and writes 3 (20 B), the correction reads 4 and writes 2 (24 B): HBM-bound, and laid out as stream.h describes, the 16-byte
// path taken whenever the row length (or n) is a multiple of 4.  The per-sample launches use the row grid of rowsum.h; the
// workspace of the loss's partial sums is its [B, parts(B, inner)] float64 layout, which stk_edm_ws_bytes states without
// seeing a pointer.  B inner < 2^31 and n < 2^31 (checked by the entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
// stream.h, included before it, holds loads, stores and host code only; sqloss.h (the loss, finish and gradient kernels shared
// with consistency.hip and flow.hip, on the scaffold of rowsum.h) holds arithmetic and follows the pragma.
#include "stream.h"
#include "stk_edm.h"

#pragma clang fp contract(off)

#include "sqloss.h"

namespace {

// One thread per sample; float64 in the header's order, each row rounded to fp32 once.
__global__ __launch_bounds__(256) void edm_coeffs_kernel(const float* sigma, double d, float* coef, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double S = (double)sigma[b];
  const double v = S * S + d * d;
  const double q = sqrt(v);
  const double p = S * d;
  coef[b] = (float)(1. / q);
  coef[(size_t)B + b] = (float)(S / q);
  coef[2 * (size_t)B + b] = (float)((d * d) / v);
  coef[3 * (size_t)B + b] = (float)(p / q);
  coef[4 * (size_t)B + b] = (float)(v / (p * p));
  coef[5 * (size_t)B + b] = (float)(log(S) / 4.);
}

// r = c_skip (y + sigma n) + c_out F - y, every operation rounded to fp32 in that order.
struct EdmRes {
  static constexpr int N = 3;
  const float* in[N];                                      // F, y, n
  const float* sigma; const float* coef;
  struct Row { float sg, csk, cou; };
  __device__ Row row(int b, int B) const { return {sigma[b], coef[2 * (size_t)B + b], coef[3 * (size_t)B + b]}; }
  __device__ static float r(const Row& c, const float* v) {
    const float x = v[1] + c.sg * v[2];
    const float D = c.csk * x + c.cou * v[0];
    return D - v[1];
  }
};

// The row's sum times lambda, rounded once.
struct EdmFinish {
  const float* coef; float* loss;
  double inner;
  int reduce_mean;
  __device__ void operator()(double acc, int b, int B) const {
    const double v = (double)coef[4 * (size_t)B + b] * acc;
    loss[b] = (float)(reduce_mean ? v / inner : v);
  }
};

struct EdmGradFactor {
  const float* coef; const float* dloss;
  float inner;
  int reduce_mean;
  __device__ float operator()(int b, int B) const {
    float k = ((2.f * coef[4 * (size_t)B + b]) * coef[3 * (size_t)B + b]) * dloss[b];
    if (reduce_mean) k = k / inner;
    return k;
  }
};

struct ChurnArgs {
  const float* x; const float* eps;
  float* x_hat; float* xin;
  float c_eps, c_in_hat;
};

// total: items of V elements.  The stride is at most 2^19 items, so i + stride stays below 2^32.
template <int V>
__global__ __launch_bounds__(256) void edm_churn_kernel(unsigned total, ChurnArgs a) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto xv = Vec<V>::load(a.x, i);
    Vec<V> ev, xh, xi;
    if (a.eps) ev = Vec<V>::load(a.eps, i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      xh.v[j] = a.eps ? xv.v[j] + a.c_eps * ev.v[j] : xv.v[j];
      xi.v[j] = a.c_in_hat * xh.v[j];
    }
    if (a.x_hat) xh.store(a.x_hat, i);
    xi.store(a.xin, i);
  }
}

struct StepArgs {
  const float* xb; const float* xe; const float* F; const float* d_prev;
  float* x_out; float* d_out; float* xin_out;
  float cs, co, t, h, c_next;
};

template <int V>
__global__ __launch_bounds__(256) void edm_step_kernel(unsigned total, StepArgs a) {
  const unsigned stride = gridDim.x * 256;
  const bool same = a.xe == a.xb;                        // the Euler stage: one read serves both
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto bv = Vec<V>::load(a.xb, i);
    const auto Fv = Vec<V>::load(a.F, i);
    Vec<V> ev = bv, pv;
    if (!same) ev = Vec<V>::load(a.xe, i);
    if (a.d_prev) pv = Vec<V>::load(a.d_prev, i);
    Vec<V> xo, dv, xi;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float D = a.cs * ev.v[j] + a.co * Fv.v[j];
      const float dn = (ev.v[j] - D) / a.t;
      const float slope = a.d_prev ? 0.5f * pv.v[j] + 0.5f * dn : dn;
      xo.v[j] = bv.v[j] + a.h * slope;
      dv.v[j] = dn;
      xi.v[j] = a.c_next * xo.v[j];
    }
    xo.store(a.x_out, i);
    if (a.d_out) dv.store(a.d_out, i);
    if (a.xin_out) xi.store(a.xin_out, i);
  }
}

}  // namespace

extern "C" int stk_edm_coeffs_f32(const float* sigma, float sigma_data, float* coef, int B, void* stream) {
  if (!sigma || !coef || B <= 0 || !stk_positive_finite(sigma_data)) return STK_EINVAL;
  hipLaunchKernelGGL(edm_coeffs_kernel, dim3(stk_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, sigma, (double)sigma_data,
                     coef, B);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" long stk_edm_ws_bytes(int B, long inner) {
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return stk_row_ws_bytes(B, inner);
}

extern "C" int stk_edm_loss_f32(const float* F, const float* y, const float* n, const float* sigma, const float* coef, void* ws,
                                long ws_bytes, float* r_out, float* loss_out, int B, long inner, int reduce_mean, void* stream) {
  if (!F || !y || !n || !sigma || !coef || !ws || !loss_out) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, B, inner)) return STK_EINVAL;
  return sq_loss_launch(stk_row_plan(B, inner, F, y, n, r_out), B, EdmRes{{F, y, n}, sigma, coef},
                        EdmFinish{coef, loss_out, (double)inner, reduce_mean}, r_out, ws, (hipStream_t)stream);
}

extern "C" int stk_edm_loss_grad_f32(const float* r, const float* coef, const float* dloss, float* dF, int B, long inner,
                                     int reduce_mean, void* stream) {
  if (!r || !coef || !dloss || !dF) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return sq_loss_grad_launch(B, inner, EdmGradFactor{coef, dloss, (float)inner, reduce_mean}, r, dF, (hipStream_t)stream);
}

extern "C" int stk_edm_churn_f32(const float* x, const float* eps, float c_eps, float c_in_hat, float* x_hat_out, float* xin_out,
                                 long n, void* stream) {
  if (!x || !xin_out || !(c_eps >= 0.f)) return STK_EINVAL;
  if (eps ? !x_hat_out : c_eps != 0.f) return STK_EINVAL;
  const int rc = stk_length_check(n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, eps, x_hat_out, xin_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  ChurnArgs a{x, eps, x_hat_out, xin_out, c_eps, c_in_hat};
  return stk_launch_vec(vec, edm_churn_kernel<4>, edm_churn_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}

extern "C" int stk_edm_step_f32(const float* xb, const float* xe, const float* F, const float* d_prev, float cs, float co, float t,
                                float h, float c_next, float* x_out, float* d_out, float* xin_out, long n, void* stream) {
  if (!xb || !xe || !F || !x_out || !stk_positive_finite(t)) return STK_EINVAL;
  const int rc = stk_length_check(n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(xb, xe, F, d_prev, x_out, d_out, xin_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  StepArgs a{xb, xe, F, d_prev, x_out, d_out, xin_out, cs, co, t, h, c_next};
  return stk_launch_vec(vec, edm_step_kernel<4>, edm_step_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}
