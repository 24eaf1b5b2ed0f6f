// consistency.hip -- the element-wise launches of consistency training and sampling (include/stk_consistency.h, gfx950): the
// per-sample coefficients of a pair of levels, both network inputs of the pair, the pseudo-Huber loss between the two
// evaluations with its gradient, and the sampler's step.
//
// Everything but the coefficients streams once over the [B, inner] batch or the n-element state -- pair reads 2 and writes 2
// tensors (8 + 8 B per element, where two stk_perturb_f32 launches move 24), loss reads 4 and writes 1 (16 + 4 B), loss_grad
// reads 1 and writes 1 (4 + 4 B), a step with noise reads 3 and writes 2-3 (20-24 B), the last step reads 2 and writes 1 (12 B):
// HBM-bound, and laid out as stream.h describes, the 16-byte path taken whenever the row length (or n) is a multiple of 4.
// The per-sample launches use the row grid of rowsum.h; the workspace of the loss's partial sums is its [B, parts(B, inner)]
// float64 layout, which stk_ct_ws_bytes states without seeing a pointer.  B inner < 2^31 and n < 2^31 (checked by the
// entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
// stream.h, included before it, holds loads, stores and host code only; sqloss.h (the loss, finish and gradient kernels shared
// with edm.hip, on the scaffold of rowsum.h) holds arithmetic and follows the pragma.
#include "stream.h"
#include "stk_consistency.h"

#pragma clang fp contract(off)

#include "sqloss.h"

namespace {

// The five rows of one level, float64 in the header's order, each rounded to fp32 once.
__device__ __forceinline__ void ct_level_rows(double S, double d, double e, float* coef, size_t B, int b) {
  const double v = S * S + d * d;
  const double q = sqrt(v);
  const double g = S - e;
  const double w = g * g + d * d;
  coef[b] = (float)(1. / q);
  coef[B + b] = (float)(S / q);
  coef[2 * B + b] = (float)((d * d) / w);
  coef[3 * B + b] = (float)((d * g) / q);
  coef[4 * B + b] = (float)(log(S) / 4.);
}

// One thread per sample.
__global__ __launch_bounds__(256) void ct_coeffs_kernel(const float* sigma_hi, const float* sigma_lo, double d, double e,
                                                        float* coef, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double Sh = (double)sigma_hi[b], Sl = (double)sigma_lo[b];
  ct_level_rows(Sh, d, e, coef, (size_t)B, b);
  ct_level_rows(Sl, d, e, coef + 5 * (size_t)B, (size_t)B, b);
  coef[10 * (size_t)B + b] = (float)(1. / (Sh - Sl));
}

struct PairArgs {
  const float* y; const float* n; const float* coef;
  float* xin_hi; float* xin_lo;
};

// row: items of V elements per sample.
template <int V>
__global__ __launch_bounds__(256) void ct_pair_kernel(unsigned row, int B, PairArgs a) {
  row_samples(B, [&](int b) {
    const float ah = a.coef[b], sh = a.coef[(size_t)B + b], al = a.coef[5 * (size_t)B + b], sl = a.coef[6 * (size_t)B + b];
    row_items(row, b, [&](unsigned i) {
      const auto yv = Vec<V>::load(a.y, i);
      const auto nv = Vec<V>::load(a.n, i);
      Vec<V> oh, ol;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        oh.v[j] = ah * yv.v[j] + sh * nv.v[j];
        ol.v[j] = al * yv.v[j] + sl * nv.v[j];
      }
      oh.store(a.xin_hi, i);
      ol.store(a.xin_lo, i);
    });
  });
}

// r = f(y + sigma_hi n; sigma_hi) - f(y + sigma_lo n; sigma_lo), every operation rounded to fp32 in that order.
struct CtRes {
  static constexpr int N = 4;
  const float* in[N];                                      // F_hi, F_lo, y, n
  const float* sigma_hi; const float* sigma_lo; const float* coef;
  struct Row { float sh, sl, ckh, coh, ckl, col; };
  __device__ Row row(int b, int B) const {
    return {sigma_hi[b], sigma_lo[b], coef[2 * (size_t)B + b], coef[3 * (size_t)B + b], coef[7 * (size_t)B + b],
            coef[8 * (size_t)B + b]};
  }
  __device__ static float r(const Row& c, const float* v) {
    const float xh = v[2] + c.sh * v[3];
    const float fh = c.ckh * xh + c.coh * v[0];
    const float xl = v[2] + c.sl * v[3];
    const float fl = c.ckl * xl + c.col * v[1];
    return fh - fl;
  }
};

// The pseudo-Huber value of the row's sum in its cancellation-free form and the factor of the gradient, each rounded once.
struct CtFinish {
  const float* coef; float* loss; float* gfac;
  double C, inner;
  int reduce_mean;
  __device__ void operator()(double acc, int b, int B) const {
    const double L = (double)coef[10 * (size_t)B + b];
    const double h = sqrt(acc + C * C);
    const double v = (L * acc) / (h + C);
    loss[b] = (float)(reduce_mean ? v / inner : v);
    if (gfac) {
      const double g = (L * (double)coef[3 * (size_t)B + b]) / h;
      gfac[b] = (float)(reduce_mean ? g / inner : g);
    }
  }
};

struct CtGradFactor {
  const float* gfac; const float* dloss;
  __device__ float operator()(int b, int B) const { return gfac[b] * dloss[b]; }
};

struct StepArgs {
  const float* x; const float* F; const float* z;
  float* x0_out; float* x_out; float* xin_out;
  float cs, co, lo, hi, c_z, c_in_next;
};

// total: items of V elements.  The stride is at most 2^19 items, so i + stride stays below 2^32.
template <int V>
__global__ __launch_bounds__(256) void ct_step_kernel(unsigned total, StepArgs a) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto xv = Vec<V>::load(a.x, i);
    const auto Fv = Vec<V>::load(a.F, i);
    Vec<V> zv, x0, xo, xi;
    if (a.z) zv = Vec<V>::load(a.z, i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float v = a.cs * xv.v[j] + a.co * Fv.v[j];
      v = v < a.lo ? a.lo : v;
      v = v > a.hi ? a.hi : v;
      x0.v[j] = v;
      if (a.z) {
        xo.v[j] = v + a.c_z * zv.v[j];
        xi.v[j] = a.c_in_next * xo.v[j];
      }
    }
    if (a.x0_out) x0.store(a.x0_out, i);
    if (a.z) {
      xo.store(a.x_out, i);
      xi.store(a.xin_out, i);
    }
  }
}

}  // namespace

extern "C" int stk_ct_coeffs_f32(const float* sigma_hi, const float* sigma_lo, float sigma_data, float sigma_min, float* coef,
                                 int B, void* stream) {
  if (!sigma_hi || !sigma_lo || !coef || B <= 0 || !stk_positive_finite(sigma_data)) return STK_EINVAL;
  if (!(sigma_min >= 0.f && sigma_min <= 3.402823466e38f)) return STK_EINVAL;
  hipLaunchKernelGGL(ct_coeffs_kernel, dim3(stk_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, sigma_hi, sigma_lo,
                     (double)sigma_data, (double)sigma_min, coef, B);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_ct_pair_f32(const float* y, const float* n, const float* coef, float* xin_hi, float* xin_lo, int B,
                               long inner, void* stream) {
  if (!y || !n || !coef || !xin_hi || !xin_lo) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  const StkRowPlan p = stk_row_plan(B, inner, y, n, xin_hi, xin_lo);
  PairArgs a{y, n, coef, xin_hi, xin_lo};
  return stk_launch_vec(p.vec, ct_pair_kernel<4>, ct_pair_kernel<1>, p.grid, (hipStream_t)stream, p.row, B, a);
}

extern "C" long stk_ct_ws_bytes(int B, long inner) {
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return stk_row_ws_bytes(B, inner);
}

extern "C" int stk_ct_loss_f32(const float* F_hi, const float* F_lo, const float* y, const float* n, const float* sigma_hi,
                               const float* sigma_lo, const float* coef, float c, void* ws, long ws_bytes, float* r_out,
                               float* gfac_out, float* loss_out, int B, long inner, int reduce_mean, void* stream) {
  if (!F_hi || !F_lo || !y || !n || !sigma_hi || !sigma_lo || !coef || !ws || !loss_out) return STK_EINVAL;
  if (!r_out != !gfac_out || !stk_positive_finite(c)) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, B, inner)) return STK_EINVAL;
  return sq_loss_launch(stk_row_plan(B, inner, F_hi, F_lo, y, n, r_out), B, CtRes{{F_hi, F_lo, y, n}, sigma_hi, sigma_lo, coef},
                        CtFinish{coef, loss_out, gfac_out, (double)c, (double)inner, reduce_mean}, r_out, ws, (hipStream_t)stream);
}

extern "C" int stk_ct_loss_grad_f32(const float* r, const float* gfac, const float* dloss, float* dF, int B, long inner,
                                    void* stream) {
  if (!r || !gfac || !dloss || !dF) return STK_EINVAL;
  const int rc = stk_row_check(B, inner);
  if (rc != STK_OK) return rc;
  return sq_loss_grad_launch(B, inner, CtGradFactor{gfac, dloss}, r, dF, (hipStream_t)stream);
}

extern "C" int stk_ct_step_f32(const float* x, const float* F, const float* z, float cs, float co, float lo, float hi, float c_z,
                               float c_in_next, float* x0_out, float* x_out, float* xin_out, long n, void* stream) {
  if (!x || !F || !(lo <= hi)) return STK_EINVAL;
  if (z ? (!x_out || !xin_out) : !x0_out) return STK_EINVAL;
  const int rc = stk_length_check(n);
  if (rc != STK_OK) return rc;
  if (!z) x_out = xin_out = nullptr;                               // not touched: they neither count for the alignment
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, F, z, x0_out, x_out, xin_out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  StepArgs a{x, F, z, x0_out, x_out, xin_out, cs, co, lo, hi, c_z, c_in_next};
  return stk_launch_vec(vec, ct_step_kernel<4>, ct_step_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total, a);
}
