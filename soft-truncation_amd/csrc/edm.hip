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
// stream.h, included before it, holds loads, stores and host code only.
#include "stream.h"
#include "stk_edm.h"

#pragma clang fp contract(off)

#include "rowsum.h"

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

struct LossArgs {
  const float* F; const float* y; const float* n; const float* sigma; const float* coef;
  float* r; double* ws;
};

// row: items of V elements per sample.
template <int V>
__global__ __launch_bounds__(256) void edm_loss_kernel(unsigned row, int B, LossArgs a) {
  __shared__ double red[4];
  const unsigned stride = gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float sg = a.sigma[b], csk = a.coef[2 * (size_t)B + b], cou = a.coef[3 * (size_t)B + b];
    const unsigned base = (unsigned)b * row;
    double acc = 0.;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) {
      const auto Fv = Vec<V>::load(a.F, base + i);
      const auto yv = Vec<V>::load(a.y, base + i);
      const auto nv = Vec<V>::load(a.n, base + i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float x = yv.v[j] + sg * nv.v[j];
        const float D = csk * x + cou * Fv.v[j];
        const float r = D - yv.v[j];
        const float q = r * r;
        acc += (double)q;
        o.v[j] = r;
      }
      if (a.r) o.store(a.r, base + i);
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) a.ws[(size_t)b * gridDim.x + blockIdx.x] = acc;
  }
}

// One block per sample (striding): the row's partials in index order within the fixed tree, times lambda, rounded once.
__global__ __launch_bounds__(256) void edm_loss_finish_kernel(const double* ws, const float* coef, float* loss, int B, int parts,
                                                              double inner, int reduce_mean) {
  __shared__ double red[4];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    double acc = 0.;
    for (int j = threadIdx.x; j < parts; j += 256) acc += ws[(size_t)b * parts + j];
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
      const double v = (double)coef[4 * (size_t)B + b] * acc;
      loss[b] = (float)(reduce_mean ? v / inner : v);
    }
  }
}

struct GradArgs {
  const float* r; const float* coef; const float* dloss;
  float* dF;
  float inner;
  int reduce_mean;
};

template <int V>
__global__ __launch_bounds__(256) void edm_loss_grad_kernel(unsigned row, int B, GradArgs a) {
  const unsigned stride = gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float k = ((2.f * a.coef[4 * (size_t)B + b]) * a.coef[3 * (size_t)B + b]) * a.dloss[b];
    if (a.reduce_mean) k = k / a.inner;
    const unsigned base = (unsigned)b * row;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) {
      const auto rv = Vec<V>::load(a.r, base + i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = k * rv.v[j];
      o.store(a.dF, base + i);
    }
  }
}

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

// 0, or the code every per-sample entry returns for B rows of `len` floats.
int check_sizes(int B, long len) {
  if (B <= 0 || len <= 0) return STK_EINVAL;
  if (len >= (1L << 31) || (long)B * len >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

// ... and every entry of the sampler for n elements.
int check_length(long n) {
  if (n <= 0) return STK_EINVAL;
  if (n >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

bool ws_ok(const void* ws, long ws_bytes, int B, long inner) {
  return ws && (((uintptr_t)ws) & 7) == 0 && ws_bytes >= (long)B * stk_row_parts(B, inner) * (long)sizeof(double);
}

bool positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }      // false for NaN and +inf

}  // namespace

extern "C" int stk_edm_coeffs_f32(const float* sigma, float sigma_data, float* coef, int B, void* stream) {
  if (!sigma || !coef || B <= 0 || !positive_finite(sigma_data)) return STK_EINVAL;
  hipLaunchKernelGGL(edm_coeffs_kernel, dim3(stk_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, sigma, (double)sigma_data,
                     coef, B);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" long stk_edm_ws_bytes(int B, long inner) {
  const int rc = check_sizes(B, inner);
  if (rc != STK_OK) return rc;
  return (long)B * stk_row_parts(B, inner) * (long)sizeof(double);
}

extern "C" int stk_edm_loss_f32(const float* F, const float* y, const float* n, const float* sigma, const float* coef, void* ws,
                                long ws_bytes, float* r_out, float* loss_out, int B, long inner, int reduce_mean, void* stream) {
  if (!F || !y || !n || !sigma || !coef || !ws || !loss_out) return STK_EINVAL;
  const int rc = check_sizes(B, inner);
  if (rc != STK_OK) return rc;
  if (!ws_ok(ws, ws_bytes, B, inner)) return STK_EINVAL;
  const bool vec = (inner & 3) == 0 && stk_all_aligned16(F, y, n, r_out);
  const unsigned row = (unsigned)(vec ? inner >> 2 : inner);
  const int parts = stk_row_parts(B, inner);
  const dim3 grid(parts, stk_row_rows(B, inner));                 // grid.x is the workspace's row length on either path
  LossArgs a{F, y, n, sigma, coef, r_out, (double*)ws};
  const int launched = stk_launch_vec(vec, edm_loss_kernel<4>, edm_loss_kernel<1>, grid, (hipStream_t)stream, row, B, a);
  if (launched != STK_OK) return launched;
  hipLaunchKernelGGL(edm_loss_finish_kernel, dim3(B < STK_MAX_GRID ? B : STK_MAX_GRID), dim3(256), 0, (hipStream_t)stream,
                     (const double*)ws, coef, loss_out, B, parts, (double)inner, reduce_mean);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_edm_loss_grad_f32(const float* r, const float* coef, const float* dloss, float* dF, int B, long inner,
                                     int reduce_mean, void* stream) {
  if (!r || !coef || !dloss || !dF) return STK_EINVAL;
  const int rc = check_sizes(B, inner);
  if (rc != STK_OK) return rc;
  const bool vec = (inner & 3) == 0 && stk_all_aligned16(r, dF);
  const unsigned row = (unsigned)(vec ? inner >> 2 : inner);
  const dim3 grid(stk_row_parts(B, inner), stk_row_rows(B, inner));
  GradArgs a{r, coef, dloss, dF, (float)inner, reduce_mean};
  return stk_launch_vec(vec, edm_loss_grad_kernel<4>, edm_loss_grad_kernel<1>, grid, (hipStream_t)stream, row, B, a);
}

extern "C" int stk_edm_churn_f32(const float* x, const float* eps, float c_eps, float c_in_hat, float* x_hat_out, float* xin_out,
                                 long n, void* stream) {
  if (!x || !xin_out || !(c_eps >= 0.f)) return STK_EINVAL;
  if (eps ? !x_hat_out : c_eps != 0.f) return STK_EINVAL;
  const int rc = check_length(n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, eps, x_hat_out, xin_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  ChurnArgs a{x, eps, x_hat_out, xin_out, c_eps, c_in_hat};
  return stk_launch_vec(vec, edm_churn_kernel<4>, edm_churn_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}

extern "C" int stk_edm_step_f32(const float* xb, const float* xe, const float* F, const float* d_prev, float cs, float co, float t,
                                float h, float c_next, float* x_out, float* d_out, float* xin_out, long n, void* stream) {
  if (!xb || !xe || !F || !x_out || !positive_finite(t)) return STK_EINVAL;
  const int rc = check_length(n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(xb, xe, F, d_prev, x_out, d_out, xin_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  StepArgs a{xb, xe, F, d_prev, x_out, d_out, xin_out, cs, co, t, h, c_next};
  return stk_launch_vec(vec, edm_step_kernel<4>, edm_step_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}
