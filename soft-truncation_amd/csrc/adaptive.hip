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
  const unsigned stride = gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float ca = a.coef[4 * b], cs = a.coef[4 * b + 2], cn = a.coef[4 * b + 3];
    const float cp = a.xp ? a.coef[4 * b + 1] : 0.f;
    const unsigned base = (unsigned)b * row;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) {
      const auto xv = Vec<V>::load(a.x, base + i);
      const auto sv = Vec<V>::load(a.score, base + i);
      const auto zv = Vec<V>::load(a.z, base + i);
      Vec<V> pv, o;
      if (a.xp) pv = Vec<V>::load(a.xp, base + i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float r = ca * xv.v[j];
        if (a.xp) r = r + cp * pv.v[j];
        r = r + cs * sv.v[j];
        o.v[j] = r + cn * zv.v[j];
      }
      o.store(a.out, base + i);
    }
  }
}

struct HeunArgs {
  const float* x; const float* x1; const float* x1_prev; const float* score2; const float* z; const float* coef;
  float* x2; double* ws;
  float atol, rtol;
};

template <int V>
__global__ __launch_bounds__(256) void sde_heun_error_kernel(unsigned row, int B, HeunArgs a) {
  __shared__ double red[4];
  const unsigned stride = gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float ca = a.coef[4 * b], cp = a.coef[4 * b + 1], cs = a.coef[4 * b + 2], cn = a.coef[4 * b + 3];
    const unsigned base = (unsigned)b * row;
    double acc = 0.;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) {
      const auto xv = Vec<V>::load(a.x, base + i);
      const auto x1v = Vec<V>::load(a.x1, base + i);
      const auto pv = Vec<V>::load(a.x1_prev, base + i);
      const auto sv = Vec<V>::load(a.score2, base + i);
      const auto zv = Vec<V>::load(a.z, base + i);
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
      o.store(a.x2, base + i);
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) a.ws[(size_t)b * gridDim.x + blockIdx.x] = acc;
  }
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
  const unsigned stride = gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    double acc = 0.;
    for (unsigned j = threadIdx.x; j < gridDim.x; j += 256) acc += a.ws[(size_t)b * gridDim.x + j];
    acc = block_sum_f64(acc, red);
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
    if (!accept) continue;                               // uniform over the block
    const unsigned base = (unsigned)b * row;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < row; i += stride) {
      const auto v2 = Vec<V>::load(a.x2, base + i);
      const auto v1 = Vec<V>::load(a.x1, base + i);
      v2.store(a.x, base + i);
      v1.store(a.x1_prev, base + i);
    }
  }
}

// 0, or the code every entry returns for these sizes.
int check_sizes(int B, long n) {
  if (B <= 0 || n <= 0) return STK_EINVAL;
  if (n >= (1L << 31) || (long)B * n >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

bool ws_ok(const void* ws, long ws_bytes, int B, long n) {
  return ws && (((uintptr_t)ws) & 7) == 0 && ws_bytes >= (long)B * stk_row_parts(B, n) * (long)sizeof(double);
}

}  // namespace

extern "C" long stk_sde_ws_bytes(int B, long n_per_sample) {
  const int rc = check_sizes(B, n_per_sample);
  if (rc != STK_OK) return rc;
  return (long)B * stk_row_parts(B, n_per_sample) * (long)sizeof(double);
}

extern "C" int stk_sde_stage_f32(const float* x, const float* xp, const float* score, const float* z, const float* coef,
                                 float* out, int B, long n, void* stream) {
  if (!x || !score || !z || !coef || !out) return STK_EINVAL;
  const int rc = check_sizes(B, n);
  if (rc != STK_OK) return rc;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, score, z, out, xp);
  const unsigned row = (unsigned)(vec ? n >> 2 : n);
  const dim3 grid(stk_row_parts(B, n), stk_row_rows(B, n));
  StageArgs a{x, xp, score, z, coef, out};
  return stk_launch_vec(vec, sde_stage_kernel<4>, sde_stage_kernel<1>, grid, (hipStream_t)stream, row, B, a);
}

extern "C" int stk_sde_heun_error_f32(const float* x, const float* x1, const float* x1_prev, const float* score2,
                                      const float* z, const float* coef, float atol, float rtol, float* x2, void* ws,
                                      long ws_bytes, int B, long n, void* stream) {
  if (!x || !x1 || !x1_prev || !score2 || !z || !coef || !x2 || !ws) return STK_EINVAL;
  if (!(atol >= 0.f) || !(rtol >= 0.f) || !(atol + rtol > 0.f)) return STK_EINVAL;
  const int rc = check_sizes(B, n);
  if (rc != STK_OK) return rc;
  if (!ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, x1, x1_prev, score2, z, x2);
  const unsigned row = (unsigned)(vec ? n >> 2 : n);
  const dim3 grid(stk_row_parts(B, n), stk_row_rows(B, n));
  HeunArgs a{x, x1, x1_prev, score2, z, coef, x2, (double*)ws, atol, rtol};
  return stk_launch_vec(vec, sde_heun_error_kernel<4>, sde_heun_error_kernel<1>, grid, (hipStream_t)stream, row, B, a);
}

extern "C" int stk_sde_commit_f32(float* x, float* x1_prev, const float* x2, const float* x1, const float* t, const float* h,
                                  float eps, float safety, float exponent, const void* ws, long ws_bytes, float* t_out,
                                  float* h_out, float* E_out, int* accept_out, int B, long n, void* stream) {
  if (!x || !x1_prev || !x2 || !x1 || !t || !h || !ws || !t_out || !h_out || !E_out || !accept_out) return STK_EINVAL;
  if (t_out == t || t_out == h || h_out == t || h_out == h || t_out == h_out) return STK_EINVAL;
  if (!(eps >= 0.f) || !(safety > 0.f) || !(exponent >= 0.f)) return STK_EINVAL;
  const int rc = check_sizes(B, n);
  if (rc != STK_OK) return rc;
  if (!ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(x, x1_prev, x2, x1);
  const unsigned row = (unsigned)(vec ? n >> 2 : n);
  const dim3 grid(stk_row_parts(B, n), stk_row_rows(B, n));
  CommitArgs a{x, x1_prev, x2, x1, t, h, (const double*)ws, t_out, h_out, E_out, accept_out, eps, safety, exponent, (double)n};
  return stk_launch_vec(vec, sde_commit_kernel<4>, sde_commit_kernel<1>, grid, (hipStream_t)stream, row, B, a);
}
