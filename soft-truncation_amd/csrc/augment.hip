// augment.hip -- the non-leaky geometric augmentation and the augmentation-label embedding (include/stk_augment.h, gfx950).
//
//   warp      one workgroup of 512 threads per (sample, channel) plane, the whole operator in LDS:
//               src  [H][W]            the flipped plane B                                   16 KB at 64 x 64
//               U    [2H][2W]          the 2x upsampling on its fundamental domain           64 KB
//               V    [2H+T-2][2W+T-2]  the warped 2x image with the apron the down pass reads  74 KB at T = 12
//             The row pass of the upsampling ([H][2W]) is staged in V's region, the row pass of the downsampling
//             ([2H+T-2][W]) in U's: 154 KB in all at the largest shape, one workgroup per CU there; a 32 x 32 plane takes
//             41 KB.  Each pass is one loop over its outputs with the threads along the W axis, so the LDS reads of a wave
//             are consecutive (up, warp rows of an axis-aligned map) or of stride 2 (down along W: 2-way, the pass is a
//             twelfth of the work); the bilinear gather of a rotated map conflicts as its addresses fall.
//             A plane whose row is the identity is copied (flipped) from global to global and touches no LDS.
//   embed     latency-bound launches on [B, D] with D = 4 nf <= 1024 and K = 9: one thread per output element.
// Every index is below 2^31 (checked by the entries); the plane offset is 64-bit.
#include "common.h"
#include "stk_augment.h"

#include <cmath>

// Every sum and product is rounded once and in the order the header states.
#pragma clang fp contract(off)

namespace {

constexpr int kAugMaxTaps = 12;
constexpr int kAugThreads = 512;

struct AugTaps {
  float f[kAugMaxTaps];
};

// Bext: reflection without edge repeat of an index onto [0, n).
__device__ __forceinline__ int aug_rho(int i, int n) {
  const int P = 2 * n - 2;
  int m = i % P;
  if (m < 0) m += P;
  return m < n ? m : P - m;
}

// The lattice of U onto its 2n stored values (the header derives it).
__device__ __forceinline__ int aug_sigma(int j, int n) {
  const int Q = 4 * n - 4;
  int m = j % Q;
  if (m < 0) m += Q;
  return m < 2 * n ? m : Q + 1 - m;
}

// The translation less whole periods 2(n-1) of U, into [-(n-1), n-1]; exact.
__device__ __forceinline__ float aug_reduce(float t, int n) {
  const float P = (float)(2 * n - 2), half = (float)(n - 1);
  float r = fmodf(t, P);
  if (r > half) r -= P;
  if (r < -half) r += P;
  return r;
}

// U[j] along one axis from the n values v[0], v[stride], ...: 2 sum_k f[k] Z[j + h - 1 - k] over the k whose Z is no zero.
__device__ __forceinline__ float aug_up(const float* v, int stride, int n, int j, const float* f, int T) {
  const int top = j + (T >> 1) - 1;         // Z index of tap 0
  float acc = 0.f;
  bool first = true;
  for (int k = top & 1; k < T; k += 2) {    // top - k even
    const float p = f[k] * v[aug_rho((top - k) >> 1, n) * stride];
    acc = first ? p : acc + p;
    first = false;
  }
  return 2.f * acc;
}

__device__ __forceinline__ float aug_down(const float* v, int stride, const float* f, int T) {
  float acc = f[0] * v[0];
  for (int k = 1; k < T; ++k) acc += f[k] * v[k * stride];
  return acc;
}

__global__ __launch_bounds__(kAugThreads) void aug_warp_kernel(const float* x, const float* params, AugTaps taps, int T,
                                                               float* y, int C, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float s_aug[];
  const int plane = blockIdx.x;
  const float* pr = params + (size_t)(plane / C) * 8;
  const bool fx = pr[0] != 0.f, fy = pr[1] != 0.f;
  const float a00 = pr[2], a01 = pr[3], a10 = pr[4], a11 = pr[5];
  const float* xs = x + (size_t)plane * (H * W);
  float* ys = y + (size_t)plane * (H * W);
  const int tid = threadIdx.x;

  if (a00 == 1.f && a01 == 0.f && a10 == 0.f && a11 == 1.f && pr[6] == 0.f && pr[7] == 0.f) {   // uniform per workgroup
    for (int i = tid; i < H * W; i += kAugThreads) {
      const int r = i / W, c = i - r * W;
      ys[i] = xs[(fy ? H - 1 - r : r) * W + (fx ? W - 1 - c : c)];
    }
    return;
  }

  const int W2 = 2 * W, H2 = 2 * H, VW = W2 + T - 2, VH = H2 + T - 2, h = T >> 1;
  float* src = s_aug;                  // [H][W]
  float* U = src + H * W;              // [H2][W2]; later the row pass of the downsampling, [VH][W]
  float* V = U + H2 * W2;              // [VH][VW]; before that the row pass of the upsampling, [H][W2]
  float* rows_up = V;
  float* rows_down = U;
  __shared__ float s_f[kAugMaxTaps];   // the taps: the up pass indexes them per lane
  if (tid < T) s_f[tid] = taps.f[tid];

  for (int i = tid; i < H * W; i += kAugThreads) {
    const int r = i / W, c = i - r * W;
    src[i] = xs[(fy ? H - 1 - r : r) * W + (fx ? W - 1 - c : c)];
  }
  __syncthreads();
  for (int i = tid; i < H * W2; i += kAugThreads) {
    const int r = i / W2, j = i - r * W2;
    rows_up[i] = aug_up(src + r * W, 1, W, j, s_f, T);
  }
  __syncthreads();
  for (int i = tid; i < H2 * W2; i += kAugThreads) {
    const int j = i / W2, c = i - j * W2;
    U[i] = aug_up(rows_up + c, W2, H, j, s_f, T);
  }
  __syncthreads();

  const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
  const float t0 = aug_reduce(pr[6], W), t1 = aug_reduce(pr[7], H);
  const float lim = 1073741824.f;
  for (int i = tid; i < VH * VW; i += kAugThreads) {
    const int r = i / VW, c = i - r * VW;
    const float dx = ((float)(c - (h - 1)) + 0.5f) * 0.5f - cx;      // exact: quarters below 2^8
    const float dy = ((float)(r - (h - 1)) + 0.5f) * 0.5f - cy;
    const float ux = ((a00 * dx + a01 * dy) + cx) + t0;
    const float uy = ((a10 * dx + a11 * dy) + cy) + t1;
    const float sx = fminf(fmaxf(2.f * ux - 0.5f, -lim), lim);
    const float sy = fminf(fmaxf(2.f * uy - 0.5f, -lim), lim);
    const float bx = floorf(sx), by = floorf(sy);
    const float gx = sx - bx, gy = sy - by;
    const int x0 = aug_sigma((int)bx, W), x1 = aug_sigma((int)bx + 1, W);
    const int y0 = aug_sigma((int)by, H), y1 = aug_sigma((int)by + 1, H);
    const float hx = 1.f - gx, hy = 1.f - gy;
    const float top = (hy * hx) * U[y0 * W2 + x0] + (hy * gx) * U[y0 * W2 + x1];
    const float bot = (gy * hx) * U[y1 * W2 + x0] + (gy * gx) * U[y1 * W2 + x1];
    V[i] = top + bot;
  }
  __syncthreads();
  for (int i = tid; i < VH * W; i += kAugThreads) {
    const int r = i / W, c = i - r * W;
    rows_down[i] = aug_down(V + r * VW + 2 * c, 1, s_f, T);
  }
  __syncthreads();
  for (int i = tid; i < H * W; i += kAugThreads) {
    const int r = i / W, c = i - r * W;
    ys[i] = aug_down(rows_down + 2 * r * W + c, W, s_f, T);
  }
}

__global__ __launch_bounds__(256) void aug_embed_fwd_kernel(unsigned total, unsigned D, int K, const float* t, const float* labels,
                                                            const float* Wt, float* y) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned b = i / D, j = i - b * D;
    const float* l = labels + b * (unsigned)K;
    const float* w = Wt + j * (unsigned)K;
    float acc = l[0] * w[0];
    for (int k = 1; k < K; ++k) acc += l[k] * w[k];
    y[i] = t[i] + acc;
  }
}

// nt = B D elements of gt (0: not wanted), nw = D K elements of the weight gradient (0: not wanted).
__global__ __launch_bounds__(256) void aug_embed_bwd_kernel(unsigned nt, unsigned nw, int B, unsigned K, unsigned D, const float* gy,
                                                            const float* labels, float* gt, int accumulate, float* gWt) {
  const unsigned stride = gridDim.x * 256;
  const unsigned total = nt > nw ? nt : nw;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    if (i < nt) gt[i] = accumulate ? gt[i] + gy[i] : gy[i];
    if (i < nw) {
      const unsigned j = i / K, k = i - j * K;
      float acc = gWt[i];
      for (int b = 0; b < B; ++b) acc += labels[(unsigned)b * K + k] * gy[(unsigned)b * D + j];
      gWt[i] = acc;
    }
  }
}

inline bool fits31(long a, long b) { return a * b < (1L << 31); }

}  // namespace

extern "C" int stk_aug_ok(int H, int W, int T) {
  return H >= 8 && H <= 64 && W >= 8 && W <= 64 && (H & 1) == 0 && (W & 1) == 0 && T >= 2 && T <= kAugMaxTaps && (T & 1) == 0;
}

extern "C" int stk_aug_warp_f32(const float* x, const float* params, const float* f, int T, float* y, int B, int C, int H, int W,
                                void* stream) {
  if (!x || !params || !f || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0 || T <= 0) return STK_EINVAL;
  if (!stk_aug_ok(H, W, T)) return STK_EUNSUPPORTED;
  AugTaps taps = {};
  for (int k = 0; k < T; ++k) {
    if (!std::isfinite(f[k])) return STK_EINVAL;
    taps.f[k] = f[k];
  }
  for (int k = 0; k < T / 2; ++k)
    if (f[k] != f[T - 1 - k]) return STK_EUNSUPPORTED;
  if (!fits31(B, C)) return STK_EUNSUPPORTED;
  const size_t lds = sizeof(float) * ((size_t)H * W * 5 + (size_t)(2 * H + T - 2) * (2 * W + T - 2));
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)aug_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return STK_ELAUNCH;
  hipLaunchKernelGGL(aug_warp_kernel, dim3((unsigned)(B * C)), dim3(kAugThreads), lds, (hipStream_t)stream, x, params, taps, T, y,
                     C, H, W);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_aug_embed_fwd_f32(const float* t, const float* labels, const float* Wt, float* y, int B, int K, int D,
                                     void* stream) {
  if (!t || !labels || !Wt || !y || B <= 0 || K <= 0 || D <= 0) return STK_EINVAL;
  if (!fits31(B, D) || !fits31(D, K) || !fits31(B, K)) return STK_EUNSUPPORTED;
  const unsigned total = (unsigned)B * (unsigned)D;
  hipLaunchKernelGGL(aug_embed_fwd_kernel, dim3(stk_ew_grid(total)), dim3(256), 0, (hipStream_t)stream, total, (unsigned)D, K, t,
                     labels, Wt, y);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_aug_embed_bwd_f32(const float* gy, const float* labels, float* gt, float beta, float* gWt, int B, int K, int D,
                                     void* stream) {
  if (!gy || !labels || (!gt && !gWt) || !(beta == 0.f || beta == 1.f) || B <= 0 || K <= 0 || D <= 0) return STK_EINVAL;
  if (!fits31(B, D) || !fits31(D, K) || !fits31(B, K)) return STK_EUNSUPPORTED;
  const unsigned nt = gt ? (unsigned)B * (unsigned)D : 0u;
  const unsigned nw = gWt ? (unsigned)D * (unsigned)K : 0u;
  hipLaunchKernelGGL(aug_embed_bwd_kernel, dim3(stk_ew_grid(nt > nw ? nt : nw)), dim3(256), 0, (hipStream_t)stream, nt, nw, B,
                     (unsigned)K, (unsigned)D, gy, labels, gt, beta != 0.f ? 1 : 0, gWt);
  STK_CHECK_LAUNCH();
  return STK_OK;
}
