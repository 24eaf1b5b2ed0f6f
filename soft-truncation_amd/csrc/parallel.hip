// parallel.hip -- the three launches of one iteration of the parallel-in-time sampler (include/stk_parallel.h, gfx950).
//
// The state is X[W + 1, B, n], slot-major.  The scan and the slide give one thread an element (or a float4) through all slots:
// the running sum Y lives in a register, the adds along the slots form a chain, but the loads do not -- they are issued for
// a group of GROUP slots at a time, unconditionally and with clamped slot indices, before the adds consume them (a per-slot
// branch around a load would make the compiler wait for each one).  The scan moves 16 B per element and slot (X, S, Z in,
// Y out; 12 B without noise), the slide 8 B.
//
// The scan runs on the row grid of rowsum.h: blockIdx.y walks the samples, blockIdx.x is one of the `parts` blocks that share a
// row; the workspace of partial sums is [B, W, parts] float64, which stk_picard_ws_bytes states without seeing a pointer.
// Per item and slot the squares are reduced over the wave by shuffles and added by lane 0 into the wave's own row of an LDS
// table -- no barrier per slot, no atomics -- and after ONE barrier thread j adds the four waves' sums of slot j in index order.
// (W + 1) B n < 2^31 (checked by the entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
#include "stream.h"
#include "stk_parallel.h"

#pragma clang fp contract(off)

#include "rowsum.h"

namespace {

constexpr int PICARD_MAX_W = 256;       // one thread per slot in the stride kernel and in the scan's epilogue
constexpr int GROUP = 8;                // slots whose loads are in flight together

struct ScanArgs {
  float* X; const float* S; const float* Z; const float* coef; double* ws;
  int i0, p, W;
};

// row: items of V elements per sample.
template <int V, bool NOISE>
__global__ __launch_bounds__(256) void picard_scan_kernel(unsigned row, int B, ScanArgs a) {
  __shared__ double part[4][PICARD_MAX_W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned slot = (unsigned)B * row;                 // items per slot
  const int last = a.p - 1;
  row_samples(B, [&](int b) {
    for (int j = lane; j < a.W; j += 64) part[wave][j] = 0.;
    __syncthreads();
    // the walk is uniform over the block (the shuffles below need every lane): a thread past the row's end reads the
    // row's last item, contributes nothing and stores nothing
    const unsigned stride = gridDim.x * 256;
    for (unsigned base = blockIdx.x * 256; base < row; base += stride) {
      const bool live = base + threadIdx.x < row;
      const unsigned i = (unsigned)b * row + (live ? base + threadIdx.x : row - 1);
      Vec<V> y = Vec<V>::load(a.X, i);                     // Y[0] = X[0]
      Vec<V> xc = y;                                       // X[j], as it was before this launch
      for (int j0 = 0; j0 < a.p; j0 += GROUP) {
        Vec<V> xn[GROUP], sv[GROUP], zv[GROUP];
        float c0[GROUP], c1[GROUP], c2[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
          const int jc = j0 + k < last ? j0 + k : last;    // clamped: slots >= p repeat slot p - 1 and are discarded
          const float* c = a.coef + 3 * (size_t)(a.i0 + jc);
          c0[k] = c[0];
          c1[k] = c[1];
          xn[k] = Vec<V>::load(a.X, (unsigned)(jc + 1) * slot + i);
          sv[k] = Vec<V>::load(a.S, (unsigned)jc * slot + i);
          if (NOISE) {
            c2[k] = c[2];
            zv[k] = Vec<V>::load(a.Z, (unsigned)((a.i0 + jc) % a.W) * slot + i);
          }
        }
        double e[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
          const int j = j0 + k;
          double acc = 0.;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float d = c0[k] * xc.v[v] + c1[k] * sv[k].v[v];
            if (NOISE) d = d + c2[k] * zv[k].v[v];
            y.v[v] = y.v[v] + d;                           // Y[j + 1]
            const float r = y.v[v] - xn[k].v[v];
            const float q = r * r;
            acc += (double)q;
          }
          if (live && j < a.p) y.store(a.X, (unsigned)(j + 1) * slot + i);
          xc = xn[k];
          e[k] = live ? acc : 0.;
        }
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
          double v = e[k];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
          if (lane == 0 && j0 + k + 1 < a.p) part[wave][j0 + k + 1] += v;      // err of slot j + 1 <= p - 1
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.W) {
      const int j = threadIdx.x;
      a.ws[((size_t)b * a.W + j) * gridDim.x + blockIdx.x] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
    }
    __syncthreads();
  });
}

struct StrideArgs {
  const double* ws; const double* thr; int* stride_out; double* err_out;
  int i0, p, W, B;
  unsigned parts;
};

// Thread j owns slot j: for every sample the partials of (b, j) in index order, the comparison, the largest error.
__global__ __launch_bounds__(256) void picard_stride_kernel(StrideArgs a) {
  __shared__ int converged[PICARD_MAX_W];
  const int j = threadIdx.x;
  if (j < a.W) {
    bool ok = true;
    double worst = 0.;
    if (j >= 1 && j < a.p) {
      const double thr = a.thr[a.i0 + j];
      for (int b = 0; b < a.B; ++b) {
        const double* part = a.ws + ((size_t)b * a.W + j) * a.parts;
        double e = 0.;
        for (unsigned k = 0; k < a.parts; ++k) e += part[k];
        if (!(e <= thr)) ok = false;                       // a NaN is not converged
        if (e != e || (worst == worst && e > worst)) worst = e;
      }
    }
    converged[j] = ok ? 1 : 0;
    if (a.err_out) a.err_out[j] = worst;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 1;
    while (s < a.p && converged[s]) ++s;
    *a.stride_out = s;
  }
}

// slot: items of V elements per slot.  Ascending j reads ahead of what it writes (s >= 1), a group's loads before its stores.
template <int V>
__global__ __launch_bounds__(256) void picard_slide_kernel(unsigned slot, float* X, const int* stride_dev, int p, int W) {
  int s = *stride_dev;
  s = s < 1 ? 1 : (s > p ? p : s);
  const int moved = p - s;                                 // slots 0 .. moved - 1 take X[j + s]; the rest take X[p]
  const unsigned step = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < slot; i += step) {
    const Vec<V> tail = Vec<V>::load(X, (unsigned)p * slot + i);
    for (int j0 = 0; j0 < moved; j0 += GROUP) {
      Vec<V> v[GROUP];
#pragma unroll
      for (int k = 0; k < GROUP; ++k) {
        const int src = j0 + k + s < p ? j0 + k + s : p;
        v[k] = Vec<V>::load(X, (unsigned)src * slot + i);
      }
#pragma unroll
      for (int k = 0; k < GROUP; ++k)
        if (j0 + k < moved) v[k].store(X, (unsigned)(j0 + k) * slot + i);
    }
    for (int j = moved; j <= W; ++j) tail.store(X, (unsigned)j * slot + i);
  }
}

// 0, or the code every entry returns for a window of W slots of B rows of n floats.
inline int picard_check(int W, int B, long n) {
  if (W < 1 || B <= 0 || n <= 0) return STK_EINVAL;
  if (W > PICARD_MAX_W) return STK_EUNSUPPORTED;
  if (n >= (1L << 31) || (long)B * n >= (1L << 31) || (long)(W + 1) * B * n >= (1L << 31)) return STK_EUNSUPPORTED;
  return STK_OK;
}

inline long picard_ws_bytes(int W, int B, long n) { return (long)W * stk_row_ws_bytes(B, n); }

inline bool picard_ws_ok(const void* ws, long ws_bytes, int W, int B, long n) {
  return ws && (((uintptr_t)ws) & 7) == 0 && ws_bytes >= picard_ws_bytes(W, B, n);
}

}  // namespace

extern "C" long stk_picard_ws_bytes(int W, int B, long n) {
  const int rc = picard_check(W, B, n);
  if (rc != STK_OK) return rc;
  return picard_ws_bytes(W, B, n);
}

extern "C" int stk_picard_scan_f32(float* X, const float* S, const float* Z, const float* coef, int i0, int p, int W,
                                   void* ws, long ws_bytes, int B, long n, void* stream) {
  const int rc = picard_check(W, B, n);
  if (rc != STK_OK) return rc;
  if (!X || !S || !coef || p < 1 || p > W || i0 < 0) return STK_EINVAL;
  if (!picard_ws_ok(ws, ws_bytes, W, B, n)) return STK_EINVAL;
  const StkRowPlan plan = stk_row_plan(B, n, X, S, Z);
  ScanArgs a{X, S, Z, coef, (double*)ws, i0, p, W};
  if (Z)
    return stk_launch_vec(plan.vec, picard_scan_kernel<4, true>, picard_scan_kernel<1, true>, plan.grid,
                          (hipStream_t)stream, plan.row, B, a);
  return stk_launch_vec(plan.vec, picard_scan_kernel<4, false>, picard_scan_kernel<1, false>, plan.grid,
                        (hipStream_t)stream, plan.row, B, a);
}

extern "C" int stk_picard_stride(const void* ws, long ws_bytes, const double* thr, int i0, int p, int W, int B, long n,
                                 int* stride_out, double* err_out, void* stream) {
  const int rc = picard_check(W, B, n);
  if (rc != STK_OK) return rc;
  if (!thr || !stride_out || p < 1 || p > W || i0 < 0) return STK_EINVAL;
  if (!picard_ws_ok(ws, ws_bytes, W, B, n)) return STK_EINVAL;
  StrideArgs a{(const double*)ws, thr, stride_out, err_out, i0, p, W, B, (unsigned)stk_row_parts(B, n)};
  hipLaunchKernelGGL(picard_stride_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_picard_slide_f32(float* X, const int* stride_dev, int p, int W, int B, long n, void* stream) {
  const int rc = picard_check(W, B, n);
  if (rc != STK_OK) return rc;
  if (!X || !stride_dev || p < 1 || p > W) return STK_EINVAL;
  const bool vec = (n & 3) == 0 && stk_all_aligned16(X);
  const long items = (long)B * (vec ? n >> 2 : n);
  return stk_launch_vec(vec, picard_slide_kernel<4>, picard_slide_kernel<1>, dim3(stk_ew_grid(items)), (hipStream_t)stream,
                        (unsigned)items, X, stride_dev, p, W);
}
