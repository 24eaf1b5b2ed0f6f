// cond.hip -- class conditioning and classifier-free guidance (include/stk_cond.h, gfx950).
//
// Three small launches.  The embedding pair works on the time embedding, [B, D] with D = 4 nf <= 1024 and B <= 1024: a few
// hundred KB at most, latency-bound, so the forms are the simplest that are coalesced and deterministic.  The combination
// streams a network output (12 B per element) and is laid out as stream.h describes.
//   forward   one item of V columns per thread; the row's class index is read (and decoded) per item
//   backward  one thread per element of gt AND per element of the table gradient: thread (c, j) walks the batch upward and
//             adds the rows whose index is c -- a fixed order per (class, column) whatever the grid is, no atomics
//   combine   out = c + w (c - u)
// Every index is below 2^31 (checked by the entries): 32-bit index arithmetic.
#include "stream.h"
#include "stk_cond.h"

// No fused multiply-add: c + w (c - u) is three roundings, as the header says, and w = 0 returns c whatever the compiler does.
#pragma clang fp contract(off)

namespace {

// The row of sample b: its index when that is an integer in [0, C], the null row C otherwise (NaN fails every comparison).
__device__ __forceinline__ int class_row(float f, int C) {
  return (f >= 0.f && f <= (float)C && f == truncf(f)) ? (int)f : C;
}

// total: items of V columns; per = D / V items per row.
template <int V>
__global__ __launch_bounds__(256) void class_embed_fwd_kernel(unsigned total, unsigned per, int C, const float* t,
                                                              const float* table, const float* idx, float* y) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned b = i / per, col = i - b * per;
    const unsigned row = (unsigned)class_row(idx[b], C);
    const auto tv = Vec<V>::load(t, i);
    const auto ev = Vec<V>::load(table, row * per + col);
    Vec<V> yv;
#pragma unroll
    for (int j = 0; j < V; ++j) yv.v[j] = tv.v[j] + ev.v[j];
    yv.store(y, i);
  }
}

// nt = B D elements of gt (0: not wanted), ne = (C + 1) D elements of the table gradient (0: not wanted).
__global__ __launch_bounds__(256) void class_embed_bwd_kernel(unsigned nt, unsigned ne, int B, int C, unsigned D, const float* gy,
                                                              const float* idx, float* gt, int accumulate, float* gtable) {
  const unsigned stride = gridDim.x * 256;
  const unsigned total = nt > ne ? nt : ne;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    if (i < nt) gt[i] = accumulate ? gt[i] + gy[i] : gy[i];
    if (i < ne) {
      const unsigned c = i / D, j = i - c * D;
      bool hit = false;
      float acc = 0.f;
      for (int b = 0; b < B; ++b) {
        if ((unsigned)class_row(idx[b], C) != c) continue;
        if (!hit) { acc = gtable[i]; hit = true; }
        acc += gy[(unsigned)b * D + j];
      }
      if (hit) gtable[i] = acc;
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void cfg_combine_kernel(unsigned total, const float* cond, const float* uncond, float w,
                                                          float* out) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const auto cv = Vec<V>::load(cond, i);
    const auto uv = Vec<V>::load(uncond, i);
    Vec<V> ov;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float d = cv.v[j] - uv.v[j];
      const float p = w * d;
      ov.v[j] = cv.v[j] + p;
    }
    ov.store(out, i);
  }
}

inline bool fits31(long a, long b) { return a * b < (1L << 31); }

}  // namespace

extern "C" int stk_class_embed_fwd_f32(const float* t, const float* table, const float* idx, float* y, int B, int C, int D,
                                       void* stream) {
  if (!t || !table || !idx || !y || B <= 0 || C <= 0 || D <= 0) return STK_EINVAL;
  if (!fits31(B, D) || !fits31((long)C + 1, D)) return STK_EUNSUPPORTED;
  const bool vec = (D & 3) == 0 && stk_all_aligned16(t, table, y);
  const unsigned per = (unsigned)(vec ? D >> 2 : D);
  const unsigned total = (unsigned)B * per;
  return stk_launch_vec(vec, class_embed_fwd_kernel<4>, class_embed_fwd_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream,
                        total, per, C, t, table, idx, y);
}

extern "C" int stk_class_embed_bwd_f32(const float* gy, const float* idx, float* gt, float beta, float* gtable, int B, int C,
                                       int D, void* stream) {
  if (!gy || !idx || (!gt && !gtable) || !(beta == 0.f || beta == 1.f) || B <= 0 || C <= 0 || D <= 0) return STK_EINVAL;
  if (!fits31(B, D) || !fits31((long)C + 1, D)) return STK_EUNSUPPORTED;
  const unsigned nt = gt ? (unsigned)B * (unsigned)D : 0u;
  const unsigned ne = gtable ? ((unsigned)C + 1u) * (unsigned)D : 0u;
  hipLaunchKernelGGL(class_embed_bwd_kernel, dim3(stk_ew_grid(nt > ne ? nt : ne)), dim3(256), 0, (hipStream_t)stream, nt, ne, B, C,
                     (unsigned)D, gy, idx, gt, beta != 0.f ? 1 : 0, gtable);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_cfg_combine_f32(const float* cond, const float* uncond, float w, float* out, long n, void* stream) {
  if (!cond || !uncond || !out || n <= 0 || !(w - w == 0.f)) return STK_EINVAL;
  if (n >= (1L << 31)) return STK_EUNSUPPORTED;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(cond, uncond, out);
  const unsigned total = (unsigned)(vec ? n >> 2 : n);
  return stk_launch_vec(vec, cfg_combine_kernel<4>, cfg_combine_kernel<1>, dim3(stk_ew_grid(total)), (hipStream_t)stream, total,
                        cond, uncond, w, out);
}
