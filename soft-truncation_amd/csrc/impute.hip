// impute.hip -- the data-consistency pass of the inpainting / colourisation samplers (include/stk_impute.h, gfx950).
//
// One streaming pass: per half-step it reads x, data, z and the mask and writes x and x_mean, 24 B per element with a full
// mask, and does a dozen multiply-adds per element (about thirty with the 3x3 colour mix) -- HBM-bound, and laid out as
// stream.h describes, the 16-byte path taken whenever H*W is a multiple of 4 (an item never leaves its plane).
// With the colour mix a thread needs the three channels of its pixels: it reads three planes H*W apart, each access still
// consecutive across the lanes, so nothing is transposed.  Every tensor has fewer than 2^31 elements (checked by the entry),
// so the index arithmetic is 32-bit: one unsigned division per item instead of a 64-bit one.
#include "stream.h"
#include "stk_impute.h"

namespace {

struct Mat3 { float m[9]; };   // row-major: (x M)_j = sum_i x_i m[3 i + j]

// v = u (1 - m) + known m,  xm = v (1 - m) + mean m: arithmetic, never a select (soft masks).  m == 0 gives v = u * 1 + 0,
// m == 1 gives v = 0 + known: both exact for finite operands.
__device__ __forceinline__ void blend(float u, float mean, float sz, float m, float& v, float& xm) {
  const float known = mean + sz, um = 1.f - m;
  v = u * um + known * m;
  xm = v * um + mean * m;
}

// The operands of one launch.  x_out may be x: an item reads all it needs before it writes, and no two items share an element.
struct Args {
  const float* x; const float* data; const float* z; const float* mask; const float* a; const float* s;
  float* x_out; float* xmean_out;
  unsigned C, hwv;          // channels; vector items per plane (H*W / V)
  unsigned mask_sn, mask_sc;  // mask strides of the image and the channel, in vector items (0: broadcast)
};

// Identity mix: every element on its own.  Item i is vector p of plane (n, c).
template <int V>
__global__ __launch_bounds__(256) void impute_kernel(unsigned total, Args g) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned plane = i / g.hwv, p = i - plane * g.hwv, n = plane / g.C, c = plane - n * g.C;
    const auto xv = Vec<V>::load(g.x, i);
    const auto dv = Vec<V>::load(g.data, i);
    const auto mv = Vec<V>::load(g.mask, n * g.mask_sn + c * g.mask_sc + p);
    Vec<V> zv;
    if (g.z) zv = Vec<V>::load(g.z, i);
    const float a = g.a[n], s = g.s[n];
    Vec<V> v, xm;
#pragma unroll
    for (int j = 0; j < V; ++j) blend(xv.v[j], a * dv.v[j], g.z ? s * zv.v[j] : 0.f, mv.v[j], v.v[j], xm.v[j]);
    v.store(g.x_out, i);
    if (g.xmean_out) xm.store(g.xmean_out, i);
  }
}

// Colour mix, C == 3: item i is vector p of image n; its three channels are hwv items apart.
template <int V>
__global__ __launch_bounds__(256) void impute_mix_kernel(unsigned total, Args g, Mat3 mix, Mat3 unmix) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned n = i / g.hwv, p = i - n * g.hwv, base = n * 3 * g.hwv + p, mbase = n * g.mask_sn + p;
    Vec<V> xv[3], dv[3], zv[3], mv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xv[c] = Vec<V>::load(g.x, base + c * g.hwv);
      dv[c] = Vec<V>::load(g.data, base + c * g.hwv);
      if (g.z) zv[c] = Vec<V>::load(g.z, base + c * g.hwv);
      if (c == 0 || g.mask_sc) mv[c] = Vec<V>::load(g.mask, mbase + c * g.mask_sc);
      else mv[c] = mv[0];
    }
    const float a = g.a[n], s = g.s[n];
    Vec<V> v[3], xm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float u = xv[0].v[j] * mix.m[k] + xv[1].v[j] * mix.m[3 + k] + xv[2].v[j] * mix.m[6 + k];
        const float d = dv[0].v[j] * mix.m[k] + dv[1].v[j] * mix.m[3 + k] + dv[2].v[j] * mix.m[6 + k];
        blend(u, a * d, g.z ? s * zv[k].v[j] : 0.f, mv[k].v[j], v[k].v[j], xm[k].v[j]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vec<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = v[0].v[j] * unmix.m[c] + v[1].v[j] * unmix.m[3 + c] + v[2].v[j] * unmix.m[6 + c];
      o.store(g.x_out, base + c * g.hwv);
      if (g.xmean_out) {
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = xm[0].v[j] * unmix.m[c] + xm[1].v[j] * unmix.m[3 + c] + xm[2].v[j] * unmix.m[6 + c];
        o.store(g.xmean_out, base + c * g.hwv);
      }
    }
  }
}

}  // namespace

extern "C" int stk_impute_f32(const float* x, const float* data, const float* z, const float* mask, const float* a,
                              const float* s, const float* mix, const float* unmix, float* x_out, float* xmean_out, int N,
                              int C, long HW, int mask_n, int mask_c, void* stream) {
  if (!x || !data || !mask || !a || !s || !x_out || N <= 0 || C <= 0 || HW <= 0 || !mix != !unmix) return STK_EINVAL;
  if (mix && C != 3) return STK_EUNSUPPORTED;
  if ((mask_n != 1 && mask_n != N) || (mask_c != 1 && mask_c != C)) return STK_EUNSUPPORTED;
  const long LIMIT = 1L << 31;
  if (HW >= LIMIT || (long)N * C >= LIMIT || (long)N * C * HW >= LIMIT) return STK_EUNSUPPORTED;
  const bool vec = (HW & 3) == 0 && stk_all_aligned16(x, data, mask, x_out, z, xmean_out);
  const unsigned hwv = (unsigned)(vec ? HW >> 2 : HW);
  Args g{x, data, z, mask, a, s, x_out, xmean_out, (unsigned)C, hwv,
         mask_n == 1 ? 0u : (unsigned)mask_c * hwv, mask_c == 1 ? 0u : hwv};
  hipStream_t st = (hipStream_t)stream;
  if (mix) {
    Mat3 m, u;
    for (int i = 0; i < 9; ++i) { m.m[i] = mix[i]; u.m[i] = unmix[i]; }
    const unsigned total = (unsigned)N * hwv;
    return stk_launch_vec(vec, impute_mix_kernel<4>, impute_mix_kernel<1>, dim3(stk_ew_grid(total)), st, total, g, m, u);
  }
  const unsigned total = (unsigned)N * (unsigned)C * hwv;
  return stk_launch_vec(vec, impute_kernel<4>, impute_kernel<1>, dim3(stk_ew_grid(total)), st, total, g);
}
