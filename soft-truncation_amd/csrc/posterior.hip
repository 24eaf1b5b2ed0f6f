// posterior.hip -- the four element-wise launches of a diffusion-posterior-sampling step (include/stk_posterior.h, gfx950).
//
// All four stream once over rows of the [N, n] state or of the [N, k] measurement -- tweedie reads 2 and writes 1 tensor,
// residual reads 2 and writes 1, guide_seed reads 2 and writes 1, guide_update reads 4-5 and writes 1-2: HBM-bound, and laid
// out as stream.h describes, the 16-byte path taken whenever the row length is a multiple of 4 (an item never leaves its
// row).  The grid is the row grid of rowsum.h, sized by the tensor the launch streams over; the workspace of the residual's
// partial sums is its [N, parts(N, k)] float64 layout, which stk_posterior_ws_bytes states without seeing a pointer.
// N n < 2^31 and N k < 2^31 (checked by the entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
// stream.h, included before it, holds loads, stores and host code only.
#include "stream.h"
#include "stk_posterior.h"

#pragma clang fp contract(off)

#include "rowsum.h"

namespace {

// The clamp, a NaN passing through, and the rule for its gradient: 1 strictly inside (lo, hi), 0 at a bound.
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool inside(float x0, float lo, float hi) { return lo < x0 && x0 < hi; }

struct TweedieArgs {
  const float* x; const float* score; const float* a; const float* s;
  float* x0;
  float lo, hi;
};

// row: items of V elements per sample.
template <int V>
__global__ __launch_bounds__(256) void tweedie_kernel(unsigned row, int N, TweedieArgs p) {
  row_samples(N, [&](int b) {
    const float a = p.a[b], s = p.s[b];
    const float s2 = s * s;
    row_items(row, b, [&](unsigned i) {
      const auto xv = Vec<V>::load(p.x, i);
      const auto sv = Vec<V>::load(p.score, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = clamp_keep_nan((xv.v[j] + s2 * sv.v[j]) / a, p.lo, p.hi);
      o.store(p.x0, i);
    });
  });
}

struct ResidualArgs {
  const float* y; const float* m;
  float* r; double* ws;
};

template <int V>
__global__ __launch_bounds__(256) void residual_kernel(unsigned row, int N, ResidualArgs p) {
  __shared__ double red[4];
  row_samples(N, [&](int b) {
    double acc = 0.;
    row_items(row, b, [&](unsigned i) {
      const auto yv = Vec<V>::load(p.y, i);
      const auto mv = Vec<V>::load(p.m, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float r = yv.v[j] - mv.v[j];
        const float rr = r * r;
        acc += (double)rr;
        o.v[j] = r;
      }
      o.store(p.r, i);
    });
    row_store_partial(acc, red, p.ws, b);
  });
}

struct SeedArgs {
  const float* v; const float* x0; const float* a; const float* s; const double* ws;
  float* seed; float* rnorm;
  float lo, hi;
  int parts;                 // partial sums per row of the workspace: stk_row_parts(N, k)
};

// Block 0 of a row sums the row's partials, in index order within the fixed tree, and records the norm.  No element of the
// seed depends on it (stk_guide_update_f32 reads it from rnorm), so the other blocks of the row do not repeat the sum.
template <int V>
__global__ __launch_bounds__(256) void guide_seed_kernel(unsigned row, int N, SeedArgs p) {
  __shared__ double red[4];
  row_samples(N, [&](int b) {
    if (blockIdx.x == 0) {                                 // uniform over the block
      const double acc = row_sum_partial(p.ws, b, p.parts, red);
      if (threadIdx.x == 0) p.rnorm[b] = (float)sqrt(acc);
    }
    const float a = p.a[b], s = p.s[b];
    const float c = (s * s) / a;
    row_items(row, b, [&](unsigned i) {
      const auto vv = Vec<V>::load(p.v, i);
      const auto x0 = Vec<V>::load(p.x0, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = inside(x0.v[j], p.lo, p.hi) ? c * vv.v[j] : 0.f;
      o.store(p.seed, i);
    });
  });
}

struct UpdateArgs {
  const float* xp; const float* xpm; const float* v; const float* gnet; const float* x0; const float* a; const float* rnorm;
  float* x_out; float* xmean_out;
  float zeta, lo, hi;
};

template <int V>
__global__ __launch_bounds__(256) void guide_update_kernel(unsigned row, int N, UpdateArgs p) {
  row_samples(N, [&](int b) {
    const float a = p.a[b], rn = p.rnorm[b];
    const float c = (rn > 0.f && rn <= 3.402823466e38f) ? p.zeta / rn : 0.f;      // false for NaN and +inf
    row_items(row, b, [&](unsigned i) {
      const auto xp = Vec<V>::load(p.xp, i);
      const auto vv = Vec<V>::load(p.v, i);
      const auto gn = Vec<V>::load(p.gnet, i);
      const auto x0 = Vec<V>::load(p.x0, i);
      Vec<V> xm, o, om;
      if (p.xpm) xm = Vec<V>::load(p.xpm, i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float g = inside(x0.v[j], p.lo, p.hi) ? vv.v[j] / a + gn.v[j] : gn.v[j];
        const float step = c * g;
        o.v[j] = xp.v[j] + step;
        if (p.xpm) om.v[j] = xm.v[j] + step;
      }
      o.store(p.x_out, i);
      if (p.xpm) om.store(p.xmean_out, i);
    });
  });
}

bool bounds_ok(float lo, float hi) { return lo <= hi; }      // false when either is NaN

}  // namespace

extern "C" long stk_posterior_ws_bytes(int N, long k) {
  const int rc = stk_row_check(N, k);
  if (rc != STK_OK) return rc;
  return stk_row_ws_bytes(N, k);
}

extern "C" int stk_tweedie_f32(const float* x, const float* score, const float* a, const float* s, float lo, float hi,
                               float* x0_out, int N, long n, void* stream) {
  if (!x || !score || !a || !s || !x0_out) return STK_EINVAL;
  if (!bounds_ok(lo, hi)) return STK_EINVAL;
  const int rc = stk_row_check(N, n);
  if (rc != STK_OK) return rc;
  const StkRowPlan pl = stk_row_plan(N, n, x, score, x0_out);
  TweedieArgs p{x, score, a, s, x0_out, lo, hi};
  return stk_launch_vec(pl.vec, tweedie_kernel<4>, tweedie_kernel<1>, pl.grid, (hipStream_t)stream, pl.row, N, p);
}

extern "C" int stk_residual_f32(const float* y, const float* m, float* r_out, void* ws, long ws_bytes, int N, long k,
                                void* stream) {
  if (!y || !m || !r_out || !ws) return STK_EINVAL;
  const int rc = stk_row_check(N, k);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, N, k)) return STK_EINVAL;
  const StkRowPlan pl = stk_row_plan(N, k, y, m, r_out);
  ResidualArgs p{y, m, r_out, (double*)ws};
  return stk_launch_vec(pl.vec, residual_kernel<4>, residual_kernel<1>, pl.grid, (hipStream_t)stream, pl.row, N, p);
}

extern "C" int stk_guide_seed_f32(const float* v, const float* x0, const float* a, const float* s, float lo, float hi,
                                  const void* ws, long ws_bytes, long k, float* seed_out, float* rnorm_out, int N, long n,
                                  void* stream) {
  if (!v || !x0 || !a || !s || !ws || !seed_out || !rnorm_out) return STK_EINVAL;
  if (!bounds_ok(lo, hi)) return STK_EINVAL;
  int rc = stk_row_check(N, n);
  if (rc != STK_OK) return rc;
  rc = stk_row_check(N, k);
  if (rc != STK_OK) return rc;
  if (!stk_row_ws_ok(ws, ws_bytes, N, k)) return STK_EINVAL;
  const StkRowPlan pl = stk_row_plan(N, n, v, x0, seed_out);
  SeedArgs p{v, x0, a, s, (const double*)ws, seed_out, rnorm_out, lo, hi, stk_row_parts(N, k)};
  return stk_launch_vec(pl.vec, guide_seed_kernel<4>, guide_seed_kernel<1>, pl.grid, (hipStream_t)stream, pl.row, N, p);
}

extern "C" int stk_guide_update_f32(const float* xp, const float* xpm, const float* v, const float* gnet, const float* x0,
                                    const float* a, const float* rnorm, float zeta, float lo, float hi, float* x_out,
                                    float* xmean_out, int N, long n, void* stream) {
  if (!xp || !v || !gnet || !x0 || !a || !rnorm || !x_out) return STK_EINVAL;
  if ((xpm == nullptr) != (xmean_out == nullptr)) return STK_EINVAL;
  if (!(zeta >= 0.f) || !bounds_ok(lo, hi)) return STK_EINVAL;
  const int rc = stk_row_check(N, n);
  if (rc != STK_OK) return rc;
  const StkRowPlan pl = stk_row_plan(N, n, xp, xpm, v, gnet, x0, x_out, xmean_out);
  UpdateArgs p{xp, xpm, v, gnet, x0, a, rnorm, x_out, xmean_out, zeta, lo, hi};
  return stk_launch_vec(pl.vec, guide_update_kernel<4>, guide_update_kernel<1>, pl.grid, (hipStream_t)stream, pl.row, N, p);
}
