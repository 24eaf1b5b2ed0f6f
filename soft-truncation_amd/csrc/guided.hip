// guided.hip -- dynamic thresholding and guidance rescale (include/stk_guided.h, gfx950): per-sample reductions over the
// [B, n] state, each followed by a streaming pass.
//
// Selection: a radix select on the 31 value bits of |v| in three levels of 11 + 10 + 10 bits.  Level k streams v once: a
// block zeroes its LDS histogram (2048 counts, 8 KiB), counts the elements of its stretch of the row that match the prefix
// found so far with integer LDS atomics, and adds its non-zero counts to the row's histogram of that level in the workspace
// with integer global atomics.  The workspace holds the levels as three planes, [B][2048], [B][1024] and [B][1024] counts.  The
// predict pass and a selection of all three levels zero it on the stream first (one memset); the launch that writes q, the
// last reader of planes two and three, leaves them zero again, so a selection behind a predict pass needs no memset and can
// be repeated.
// Before it counts, every block of a row finds the row's prefix itself: it scans the row's earlier histograms (8 or 4
// counts per thread, a block-wide exclusive scan, the one thread whose stretch holds the rank walks its counts).  A last
// launch of one block per row scans all three and writes q.  Counts are integers: whatever order the atomics arrive in, the
// histograms, and with them q, are the same bits on every call.
//
// The streaming kernels are laid out as stream.h describes on the row grid of rowsum.h; B n < 2^31 (checked by the
// entries), so the index arithmetic is 32-bit.
//
// No fused multiply-add in this file (header, "Arithmetic"): the pragma below holds for every function that follows.
#include "stream.h"
#include "stk_guided.h"

#pragma clang fp contract(off)

#include "rowsum.h"

namespace {

constexpr unsigned BINS1 = 2048, BINS2 = 1024, BINS3 = 1024;          // 11 + 10 + 10 bits
constexpr unsigned ROW_WORDS = BINS1 + BINS2 + BINS3;                  // 4096 counts = 16 KiB per row, in three planes
constexpr int SUMS = 4;                                                // sum c, sum c c, sum g, sum g g

__device__ __forceinline__ unsigned key_of(float f) { return __float_as_uint(f) & 0x7fffffffu; }

// Row b's histogram of level 1, 2 or 3 in the workspace of B rows: the planes [B][BINS1], [B][BINS2], [B][BINS3].
template <class T> __device__ __forceinline__ T* hist1_of(T* ws, int B, int b) { return ws + (size_t)b * BINS1; }
template <class T> __device__ __forceinline__ T* hist2_of(T* ws, int B, int b) { return ws + (size_t)B * BINS1 + (size_t)b * BINS2; }
template <class T> __device__ __forceinline__ T* hist3_of(T* ws, int B, int b) {
  return ws + (size_t)B * (BINS1 + BINS2) + (size_t)b * BINS3;
}

// The bin of hist[0..NB) that holds rank `rank` of the counted elements, and the rank inside that bin; the same in every
// thread.  The last bin and 0 when the counts sum to `rank` or less (a workspace the caller left in another state): the
// result is a valid bin whatever the counts are.  sh: 6 words of LDS.  Ends with a barrier, so sh can be reused.
template <unsigned NB>
__device__ __forceinline__ void find_bin(const unsigned* hist, unsigned rank, unsigned* sh, unsigned& bin, unsigned& within) {
  constexpr int PER = NB / 256;
  static_assert(PER == 4 || PER == 8, "one or two 16-byte loads per thread");
  const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned c[PER];
#pragma unroll
  for (int k = 0; k < PER / 4; ++k) {
    const uint4 t = reinterpret_cast<const uint4*>(hist)[tid * (PER / 4) + k];
    c[4 * k] = t.x; c[4 * k + 1] = t.y; c[4 * k + 2] = t.z; c[4 * k + 3] = t.w;
  }
  unsigned local = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) local += c[j];
  unsigned inc = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= (unsigned)o) inc += t;
  }
  if (lane == 63) sh[wid] = inc;
  if (tid == 0) { sh[4] = NB - 1; sh[5] = 0; }
  __syncthreads();
  unsigned before = inc - local;
  for (unsigned w = 0; w < wid; ++w) before += sh[w];
  if (before <= rank && rank - before < local) {                       // exactly one thread when the counts exceed rank
    unsigned r = rank - before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!found) {
        if (r < c[j]) { sh[4] = tid * PER + j; sh[5] = r; found = true; }
        else r -= c[j];
      }
    }
  }
  __syncthreads();
  bin = sh[4];
  within = sh[5];
  __syncthreads();
}

__device__ __forceinline__ void zero_hist(unsigned* hist, unsigned nb) {
  for (unsigned i = threadIdx.x; i < nb; i += 256) hist[i] = 0;
  __syncthreads();
}

// The block's counts into the row's histogram; a barrier on both sides.
__device__ __forceinline__ void flush_hist(const unsigned* hist, unsigned nb, unsigned* out) {
  __syncthreads();
  for (unsigned i = threadIdx.x; i < nb; i += 256) {
    const unsigned c = hist[i];
    if (c) atomicAdd(out + i, c);
  }
  __syncthreads();
}

// Level LEVEL (1, 2, 3) of the selection.  row: items of V elements per sample.
template <int V, int LEVEL>
__global__ __launch_bounds__(256) void select_pass_kernel(unsigned row, int B, const float* v, unsigned rank, unsigned* ws) {
  __shared__ unsigned hist[BINS1];
  __shared__ unsigned sh[6];
  constexpr unsigned NB = LEVEL == 1 ? BINS1 : (LEVEL == 2 ? BINS2 : BINS3);
  row_samples(B, [&](int b) {
    unsigned prefix = 0, r = rank, bin;
    if (LEVEL >= 2) { find_bin<BINS1>(hist1_of(ws, B, b), r, sh, bin, r); prefix = bin; }
    if (LEVEL == 3) { find_bin<BINS2>(hist2_of(ws, B, b), r, sh, bin, r); prefix = (prefix << 10) | bin; }
    zero_hist(hist, NB);
    row_items(row, b, [&](unsigned i) {
      const auto vv = Vec<V>::load(v, i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const unsigned k = key_of(vv.v[j]);
        if (LEVEL == 1) atomicAdd(&hist[k >> 20], 1u);
        if (LEVEL == 2) { if ((k >> 20) == prefix) atomicAdd(&hist[(k >> 10) & 1023u], 1u); }
        if (LEVEL == 3) { if ((k >> 10) == prefix) atomicAdd(&hist[k & 1023u], 1u); }
      }
    });
    flush_hist(hist, NB, LEVEL == 1 ? hist1_of(ws, B, b) : (LEVEL == 2 ? hist2_of(ws, B, b) : hist3_of(ws, B, b)));
  });
}

// One block per row (striding): the three scans, and q; then the row's planes two and three are zeroed for the next
// selection on the same first level.  It does not read v.
__global__ __launch_bounds__(256) void select_finish_kernel(int B, unsigned rank, unsigned* ws, float* q) {
  __shared__ unsigned sh[6];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    unsigned r = rank, b1, b2, b3;
    find_bin<BINS1>(hist1_of(ws, B, b), r, sh, b1, r);
    find_bin<BINS2>(hist2_of(ws, B, b), r, sh, b2, r);
    find_bin<BINS3>(hist3_of(ws, B, b), r, sh, b3, r);
    if (threadIdx.x == 0) q[b] = __uint_as_float((b1 << 20) | (b2 << 10) | b3);
    unsigned* h2 = hist2_of(ws, B, b);                     // find_bin ended with a barrier: every count has been read
    unsigned* h3 = hist3_of(ws, B, b);
    for (unsigned i = threadIdx.x; i < BINS2; i += 256) h2[i] = 0;
    for (unsigned i = threadIdx.x; i < BINS3; i += 256) h3[i] = 0;
  }
}

// d_raw = cx x + cs score, and the first level of the selection on |d_raw|.
template <int V>
__global__ __launch_bounds__(256) void predict_kernel(unsigned row, int B, const float* x, const float* score, float cx, float cs,
                                                      float* d_raw, unsigned* ws) {
  __shared__ unsigned hist[BINS1];
  row_samples(B, [&](int b) {
    zero_hist(hist, BINS1);
    row_items(row, b, [&](unsigned i) {
      const auto xv = Vec<V>::load(x, i);
      const auto sv = Vec<V>::load(score, i);
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float px = cx * xv.v[j];
        const float ps = cs * sv.v[j];
        o.v[j] = px + ps;
        atomicAdd(&hist[key_of(o.v[j]) >> 20], 1u);
      }
      o.store(d_raw, i);
    });
    flush_hist(hist, BINS1, hist1_of(ws, B, b));
  });
}

struct UpdateArgs {
  const float* x; const float* d_raw; const float* d_prev; const float* q;
  float* x_out; float* d_out;
  float floor, g, A, Bc;
};

// The clamp, a NaN passing through (and a NaN bound leaving v as it is: the division that follows makes the NaN).
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int V>
__global__ __launch_bounds__(256) void threshold_update_kernel(unsigned row, int B, UpdateArgs p) {
  row_samples(B, [&](int b) {
    const float qb = p.q[b];
    const float s = qb != qb ? qb : (qb > p.floor ? qb : p.floor);
    const float ms = -s;
    row_items(row, b, [&](unsigned i) {
      const auto rv = Vec<V>::load(p.d_raw, i);
      Vec<V> xv, pv, xo, dv;
      if (p.x) xv = Vec<V>::load(p.x, i);
      if (p.d_prev) pv = Vec<V>::load(p.d_prev, i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = clamp_keep_nan(rv.v[j], ms, s) / s;
        dv.v[j] = d;
        if (p.x) {
          float D = d;
          if (p.d_prev) {
            const float diff = d - pv.v[j];
            const float ext = p.g * diff;
            D = d + ext;
          }
          const float ax = p.A * xv.v[j];
          const float bd = p.Bc * D;
          xo.v[j] = ax + bd;
        }
      }
      if (p.x) xo.store(p.x_out, i);
      if (p.d_out) dv.store(p.d_out, i);
    });
  });
}

// Pass 1 of the rescale: g, and the row's partial sums [B, parts, SUMS].
template <int V>
__global__ __launch_bounds__(256) void rescale_combine_kernel(unsigned row, int B, const float* cond, const float* uncond, float w,
                                                              float* out, double* ws) {
  __shared__ double red[4];
  row_samples(B, [&](int b) {
    double acc[SUMS] = {0., 0., 0., 0.};                               // sum c, sum c c, sum g, sum g g
    row_items(row, b, [&](unsigned i) {
      const auto cv = Vec<V>::load(cond, i);
      const auto uv = Vec<V>::load(uncond, i);
      Vec<V> ov;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = cv.v[j] - uv.v[j];
        const float p = w * d;
        const float g = cv.v[j] + p;
        const double c64 = (double)cv.v[j], g64 = (double)g;
        const double cc = c64 * c64, gg = g64 * g64;                   // exact: 24-bit operands
        acc[0] += c64; acc[1] += cc; acc[2] += g64; acc[3] += gg;
        ov.v[j] = g;
      }
      ov.store(out, i);
    });
    row_store_partials(acc, red, ws, b);
  });
}

// Pass 2: every block of a row sums the row's partials itself, in the same order, and scales its stretch of g in place.
template <int V>
__global__ __launch_bounds__(256) void rescale_scale_kernel(unsigned row, int B, double n, float phi, float* out, const double* ws) {
  __shared__ double red[4];
  row_samples(B, [&](int b) {
    double s[SUMS];
    row_sum_partials(ws, b, gridDim.x, red, s);
    const double mc = s[0] / n, mg = s[2] / n;
    double vc = s[1] / n - mc * mc, vg = s[3] / n - mg * mg;
    vc = vc < 0. ? 0. : vc;
    vg = vg < 0. ? 0. : vg;
    const double sdc = sqrt(vc), sdg = sqrt(vg);
    float f = 1.f;
    if (sdg > 0. && sdg <= 1.7976931348623157e308) {                   // false for NaN and +inf
      const double ratio = sdc / sdg;
      const double scaled = (double)phi * ratio;
      f = (float)(scaled + (1. - (double)phi));
    }
    row_items(row, b, [&](unsigned i) {
      auto gv = Vec<V>::load(out, i);
#pragma unroll
      for (int j = 0; j < V; ++j) gv.v[j] = f * gv.v[j];
      gv.store(out, i);
    });
  });
}

long select_bytes(int B) { return (long)B * ROW_WORDS * (long)sizeof(unsigned); }

long ws_bytes_of(int B, long n) {
  const long a = select_bytes(B), b = stk_row_ws_bytes(B, n, SUMS);
  return a > b ? a : b;
}

bool guided_ws_ok(const void* ws, long ws_bytes, int B, long n) {
  return ws && stk_aligned16(ws) && ws_bytes >= ws_bytes_of(B, n);
}

}  // namespace

extern "C" long stk_guided_ws_bytes(int B, long n) {
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  return ws_bytes_of(B, n);
}

extern "C" int stk_abs_select_f32(const float* v, int B, long n, long rank, float* q, void* ws, long ws_bytes,
                                  int first_level_done, void* stream) {
  if (!v || !q || !ws) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  if (rank < 0 || rank >= n || (first_level_done != 0 && first_level_done != 1) || !guided_ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const StkRowPlan p = stk_row_plan(B, n, v);
  const unsigned r = (unsigned)rank;
  unsigned* w = (unsigned*)ws;
  if (!first_level_done) {
    if (hipMemsetAsync(ws, 0, (size_t)select_bytes(B), st) != hipSuccess) return STK_ELAUNCH;
    const int rc1 = stk_launch_vec(p.vec, select_pass_kernel<4, 1>, select_pass_kernel<1, 1>, p.grid, st, p.row, B, v, r, w);
    if (rc1 != STK_OK) return rc1;
  }
  const int rc2 = stk_launch_vec(p.vec, select_pass_kernel<4, 2>, select_pass_kernel<1, 2>, p.grid, st, p.row, B, v, r, w);
  if (rc2 != STK_OK) return rc2;
  const int rc3 = stk_launch_vec(p.vec, select_pass_kernel<4, 3>, select_pass_kernel<1, 3>, p.grid, st, p.row, B, v, r, w);
  if (rc3 != STK_OK) return rc3;
  hipLaunchKernelGGL(select_finish_kernel, dim3(B < STK_MAX_GRID ? B : STK_MAX_GRID), dim3(256), 0, st, B, r, w, q);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

extern "C" int stk_dpm_predict_f32(const float* x, const float* score, float cx, float cs, float* d_raw, int B, long n, void* ws,
                                   long ws_bytes, void* stream) {
  if (!x || !score || !d_raw || !ws) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  if (!guided_ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const StkRowPlan p = stk_row_plan(B, n, x, score, d_raw);
  if (hipMemsetAsync(ws, 0, (size_t)select_bytes(B), st) != hipSuccess) return STK_ELAUNCH;
  return stk_launch_vec(p.vec, predict_kernel<4>, predict_kernel<1>, p.grid, st, p.row, B, x, score, cx, cs, d_raw, (unsigned*)ws);
}

extern "C" int stk_dpm_threshold_update_f32(const float* x, const float* d_raw, const float* d_prev, const float* q, float floor,
                                            float g, float A, float Bc, float* x_out, float* d_out, int B, long n, void* stream) {
  if (!d_raw || !q || (x == nullptr) != (x_out == nullptr) || (!x && !d_out)) return STK_EINVAL;
  if ((g != 0.f && !d_prev) || !(floor > 0.f && floor <= 3.402823466e38f)) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  const StkRowPlan pl = stk_row_plan(B, n, x, d_raw, d_prev, x_out, d_out);
  UpdateArgs p{x, d_raw, d_prev, q, x_out, d_out, floor, g, A, Bc};
  return stk_launch_vec(pl.vec, threshold_update_kernel<4>, threshold_update_kernel<1>, pl.grid, (hipStream_t)stream, pl.row, B, p);
}

extern "C" int stk_cfg_rescale_f32(const float* cond, const float* uncond, float w, float phi, float* out, int B, long n, void* ws,
                                   long ws_bytes, void* stream) {
  if (!cond || !uncond || !out || !ws || !(w - w == 0.f) || !(phi >= 0.f && phi <= 1.f)) return STK_EINVAL;
  const int rc = stk_row_check(B, n);
  if (rc != STK_OK) return rc;
  if (!guided_ws_ok(ws, ws_bytes, B, n)) return STK_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const StkRowPlan p = stk_row_plan(B, n, cond, uncond, out);
  const int rc1 = stk_launch_vec(p.vec, rescale_combine_kernel<4>, rescale_combine_kernel<1>, p.grid, st, p.row, B, cond, uncond, w,
                                 out, (double*)ws);
  if (rc1 != STK_OK) return rc1;
  return stk_launch_vec(p.vec, rescale_scale_kernel<4>, rescale_scale_kernel<1>, p.grid, st, p.row, B, (double)n, phi, out,
                        (const double*)ws);
}
