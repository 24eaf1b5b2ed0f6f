// adaptive.hip -- the three passes of the adaptive-step SDE sampler (include/stk_adaptive.h, gfx950).
//
// All three stream over the [B, n] state once -- stage reads 3-4 and writes 1 tensor, heun_error reads 5 and writes 1, commit
// reads 2 and writes 2 for the accepted rows only: HBM-bound, and laid out as stream.h describes, the 16-byte path taken
// whenever n is a multiple of 4 (an item never leaves its row).
//
// The grid is the row grid of rowsum.h: blockIdx.y walks the samples, blockIdx.x is one of the `parts` blocks that share a row;
// the workspace of partial sums is its [B, parts] float64 layout, which stk_sde_ws_bytes states without seeing a pointer.
// B n < 2^31 (checked by the entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
// stream.h, included before it, holds loads, stores and host code only.
#include "stream.h"
#include "stk_adaptive.h"

#pragma clang fp contract(off)

#include "rowsum.h"

namespace {

struct StageArgs {
  const float* x; const float* xp; const float* score; const float* z; const float* coef;
  float* out;
};

// row: items of V elements per sample.
template <int V>
__global__ __launch_bounds__(256) void sde_stage_kernel(unsigned row, int B, StageArgs a) {
  row_samples(B, [&](int b) {
    const float ca = a.coef[4 * b], cs = a.coef[4 * b + 2], cn = a.coef[4 * b + 3];
    const float cp = a.xp ? a.coef[4 * b + 1] : 0.f;
    row_items(row, b, [&](unsigned i) {
      const auto xv = Vec<V>::load(a.x, i);
      const auto sv = Vec<V>::load(a.score, i);
      const auto zv = Vec<V>::load(a.z, i);
      Vec<V> pv, o;
      if (a.xp) pv = Vec<V>::load(a.xp, i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float r = ca * xv.v[j];
        if (a.xp) r = r + cp * pv.v[j];
        r = r + cs * sv.v[j];
        o.v[j] = r + cn * zv.v[j];
      }
      o.store(a.out, i);
    });
  });
}

struct HeunArgs {
  const float* x; const float* x1; const float* x1_prev; const float* score2; const float* z; const float* coef;
  float* x2; double* ws;
  float atol, rtol;
};

template <int V>
__global__ __launch_bounds__(256) void sde_heun_error_kernel(unsigned row, int B, HeunArgs a) {
  __shared__ double red[4];
  row_samples(B, [&](int b) {
    const float ca = a.coef[4 * b], cp = a.coef[4 * b + 1], cs = a.coef[4 * b + 2], cn = a.coef[4 * b + 3];
    double acc = 0.;
    row_items(row, b, [&](unsigned i) {
      const auto xv = Vec<V>::load(a.x, i);
      const auto x1v = Vec<V>::load(a.x1, i);
      const auto pv = Vec<V>::load(a.x1_prev, i);
      const auto sv = Vec<V>::load(a.score2, i);
      const auto zv = Vec<V>::load(a.z, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float x1 = x1v.v[j];
        const float xt = ((ca * xv.v[j] + cp * x1) + cs * sv.v[j]) + cn * zv.v[j];
        const float x2 = 0.5f * (x1 + xt);
        const float d = fmaxf(a.atol, a.rtol * fmaxf(fabsf(x1), fabsf(pv.v[j])));
        const float q = (x1 - x2) / d;
        const float qq = q * q;
        acc += (double)qq;
        o.v[j] = x2;
      }
      o.store(a.x2, i);
    });
    row_store_partial(acc, red, a.ws, b);
  });
}

struct CommitArgs {
  float* x; float* x1_prev; const float* x2; const float* x1; const float* t; const float* h; const double* ws;
  float* t_out; float* h_out; float* E_out; int* accept_out;
  float eps, safety, exponent;
  double n;
};

// Every block of a row sums the row's partials itself, in the same order: all of them reach the same E and the same
// decision without reading anything another block of this launch writes.  Block 0 of the row records the decision.
template <int V>
__global__ __launch_bounds__(256) void sde_commit_kernel(unsigned row, int B, CommitArgs a) {
  __shared__ double red[4];
  row_samples(B, [&](int b) {
    const double acc = row_sum_partial(a.ws, b, gridDim.x, red);
    const float E = sqrtf((float)(acc / a.n));
    const float t = a.t[b], h = a.h[b];
    const bool active = t > a.eps;
    const bool finite = E <= 3.402823466e38f;           // false for NaN and +inf (E is never negative)
    const bool accept = active && E <= 1.f;
    const float t_step = h >= t - a.eps ? a.eps : t - h;
    const float t_new = accept ? t_step : t;
    float h_new = 0.f;
    if (active) {
      const double next = finite ? (double)a.safety * (double)h * pow((double)E, -(double)a.exponent)
                                 : (double)a.safety * (double)h * 0.5;
      h_new = fminf(t_new - a.eps, (float)next);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.t_out[b] = t_new;
      a.h_out[b] = h_new;
      a.E_out[b] = E;
      a.accept_out[b] = accept ? 1 : 0;
    }
    if (accept) {                                        // uniform over the block
      row_items(row, b, [&](unsigned i) {
        const auto v2 = Vec<V>::load(a.x2, i);
        const auto v1 = Vec<V>::load(a.x1, i);
        v2.store(a.x, i);
        v1.store(a.x1_prev, i);
      });
    }
  });
}

}  // namespace

extern "C" long stk_sde_ws_bytes(int B, long n_per_sample) {
  const int rc = stk_row_check(B, n_per_sample);
  if (rc != STK_OK) return rc;
  return stk_row_ws_bytes(B, n_per_sample);
}

extern "C" int stk_sde_stage_f32(const float* x, const float* xp, const float* score, const float* z, const float* coef,
                                 float* out, int B, long n, void* stream) {
  if (!x || !score || !z || !coef || !out) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  const StkRowPlan p = stk_row_plan(B, n, x, score, z, out, xp);
  StageArgs a{x, xp, score, z, coef, out};
  return stk_launch_vec(p.vec, sde_stage_kernel<4>, sde_stage_kernel<1>, p.grid, (hipStream_t)stream, p.row, B, a);
}

extern "C" int stk_sde_heun_error_f32(const float* x, const float* x1, const float* x1_prev, const float* score2,
                                      const float* z, const float* coef, float atol, float rtol, float* x2, void* ws,
                                      long ws_bytes, int B, long n, void* stream) {
  if (!x || !x1 || !x1_prev || !score2 || !z || !coef || !x2 || !ws) return STK_EINVAL;
  if (!(atol >= 0.f) || !(rtol >= 0.f) || !(atol + rtol > 0.f)) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const StkRowPlan p = stk_row_plan(B, n, x, x1, x1_prev, score2, z, x2);
  HeunArgs a{x, x1, x1_prev, score2, z, coef, x2, (double*)ws, atol, rtol};
  return stk_launch_vec(p.vec, sde_heun_error_kernel<4>, sde_heun_error_kernel<1>, p.grid, (hipStream_t)stream, p.row, B, a);
}

extern "C" int stk_sde_commit_f32(float* x, float* x1_prev, const float* x2, const float* x1, const float* t, const float* h,
                                  float eps, float safety, float exponent, const void* ws, long ws_bytes, float* t_out,
                                  float* h_out, float* E_out, int* accept_out, int B, long n, void* stream) {
  if (!x || !x1_prev || !x2 || !x1 || !t || !h || !ws || !t_out || !h_out || !E_out || !accept_out) return STK_EINVAL;
  if (t_out == t || t_out == h || h_out == t || h_out == h || t_out == h_out) return STK_EINVAL;
  if (!(eps >= 0.f) || !(safety > 0.f) || !(exponent >= 0.f)) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const StkRowPlan p = stk_row_plan(B, n, x, x1_prev, x2, x1);
  CommitArgs a{x, x1_prev, x2, x1, t, h, (const double*)ws, t_out, h_out, E_out, accept_out, eps, safety, exponent, (double)n};
  return stk_launch_vec(p.vec, sde_commit_kernel<4>, sde_commit_kernel<1>, p.grid, (hipStream_t)stream, p.row, B, a);
}
