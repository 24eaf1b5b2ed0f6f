// superres.hip -- the data-consistency pass of the super-resolution sampler (include/stk_superres.h, gfx950): the r x r block
// means of the state are replaced by the perturbed measurement, every pixel of a block receiving the same shift.
//
// HBM-bound: per launch x is read once and each output written once, 3 + 2/P state-sized tensors (2 + 2/P without x_mean;
// low and z are 1/P of the state each, P = r^2).  The first add-on kernel that is not element-wise: it needs a sum over each
// block and a broadcast back, and does both in registers.
//
// 16-byte path (stream.h; every pointer 16-byte aligned and W a multiple of 4).  An item is (plane, block row, column quad),
// flattened in that order, so the lanes of a wave walk consecutive float4s of a row.  A lane loads the r float4s of its
// column quad, W apart, and keeps them (64 VGPRs at r = 16); adds them down the rows (r - 1 additions per column); adds the
// four columns of its quad as (c0 + c1) + (c2 + c3) -- at r = 2 the two pairs are two blocks -- and, at r = 8 and 16, adds the
// partial sums of the 2 or 4 adjacent lanes that share a block with an xor butterfly (__shfl_xor 1, then 2; no LDS).  The add
// is commutative, so both sides of an exchange compute the same bits: every pixel of a block gets the same m_x.  Lane groups
// are aligned: W/4 is a multiple of r/4 and the block and grid strides are multiples of 256, so an item's position in its
// group is that of its lane, and a group is in range or out of range as a whole.  Every lane of a wave reaches the exchange:
// the grid-stride loop runs over block bases (a trip count uniform in the block), and only the loads and stores of an item
// past the end are guarded.  x_out may be x: an item reads all it needs before it writes, and no two items share an element.
//
// d, the number of additions on the longest path from an element of x to its block sum, is
//     d = (r - 1) + log2 r          (2, 5, 10, 19 for r = 2, 4, 8, 16)
// on both paths: r - 1 down the rows, then a balanced tree over the r columns.  The scaling by 1/P is exact.
//
// Scalar path (a pointer not 16-byte aligned, or W % 4 != 0, which only r = 2 allows).  An item is one block; its thread sums
// the block in the same order (column sums down the rows, then the same tree, hence the same bits as the 16-byte path), then
// walks the block again to write.  Correct, not fast: adjacent lanes are r floats apart, so a wave's load touches 64 segments
// of 4 bytes with a stride of 4 r bytes and every cache line is visited by r load instructions per row; x is read twice, the
// second time from cache at best; and the r^2 loads of a block are serial in one lane instead of spread over r/4 lanes.
//
// No fused multiply-add in this file: with z == NULL x_out and x_mean must be bit-identical, and a * low contracted into one
// of the two subtractions and not the other would break that.  The pragma below holds for every function that follows;
// stream.h, included before it, holds loads, stores and host code only.
#include "stream.h"
#include "stk_superres.h"

#pragma clang fp contract(off)

namespace {

// The operands of one launch.  Every tensor has fewer than 2^31 elements (checked by the entries): 32-bit index arithmetic.
struct Args {
  const float* x; const float* low; const float* z; const float* a; const float* s;
  float* x_out; float* xmean_out;
  unsigned C, hb, wu;       // channels; block rows per plane (H / r); row length in items (W / 4, or W / r on the scalar path)
};

// Balanced tree over c[0..n): ((c0 + c1) + (c2 + c3)) + ...; n a power of two.
template <int n>
__device__ __forceinline__ float tree_sum(const float* c) {
  if constexpr (n == 1) return c[0];
  else return tree_sum<n / 2>(c) + tree_sum<n / 2>(c + n / 2);
}

// The block means a lane's column quad belongs to, from the r float4s it holds: m[0] for columns 0-1, m[1] for columns 2-3
// (two blocks at r = 2, the same one otherwise).  Executed by every lane of the wave.
template <int R>
__device__ __forceinline__ void quad_means(const Vec<4> (&rows)[R], float (&m)[2]) {
  float c[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k] = rows[0].v[k];
#pragma unroll
    for (int j = 1; j < R; ++j) c[k] += rows[j].v[k];
  }
  constexpr float inv_p = 1.f / (R * R);
  if constexpr (R == 2) {
    m[0] = (c[0] + c[1]) * inv_p;
    m[1] = (c[2] + c[3]) * inv_p;
  } else {
    float t = (c[0] + c[1]) + (c[2] + c[3]);
    if constexpr (R >= 8) t += __shfl_xor(t, 1, 64);
    if constexpr (R >= 16) t += __shfl_xor(t, 2, 64);
    m[0] = m[1] = t * inv_p;
  }
}

// The r float4s of item i (zeros past the end), and where the item sits: rg = plane * hb + block row, q = its column quad.
template <int R>
__device__ __forceinline__ void load_quad(const float* x, unsigned i, bool live, unsigned wq, Vec<4> (&rows)[R], unsigned& rg,
                                          unsigned& q) {
  rg = i / wq;
  q = i - rg * wq;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (live) rows[j] = Vec<4>::load(x, (rg * R + j) * wq + q);
    else rows[j] = Vec<4>{{0.f, 0.f, 0.f, 0.f}};
  }
}

// The one or two values of a [.., H/r, W/r] tensor that item (rg, q) needs: element rg * (W/r) + the block column(s) of q.
template <int R>
__device__ __forceinline__ void load_low(const float* p, unsigned rg, unsigned q, unsigned wq, float (&v)[2]) {
  if constexpr (R == 2) {
    const float2 t = reinterpret_cast<const float2*>(p)[rg * wq + q];      // W/2 = 2 wq values per row: 8-byte aligned
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = v[1] = p[rg * (wq / (R / 4)) + q / (R / 4)];
  }
}

template <int R>
__global__ __launch_bounds__(256) void superres_vec_kernel(unsigned total, Args g) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned base = blockIdx.x * 256; base < total; base += stride) {
    const unsigned i = base + threadIdx.x;
    const bool live = i < total;
    Vec<4> rows[R];
    unsigned rg, q;
    load_quad<R>(g.x, i, live, g.wu, rows, rg, q);
    float m[2];
    quad_means<R>(rows, m);
    if (!live) continue;
    const unsigned n = rg / g.hb / g.C;
    const float a = g.a[n], sr = g.s[n] * (1.f / R);
    float lo[2], zz[2], dk[2], dm[2];
    load_low<R>(g.low, rg, q, g.wu, lo);
    if (g.z) load_low<R>(g.z, rg, q, g.wu, zz);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float mean = a * lo[h];
      const float known = g.z ? mean + sr * zz[h] : mean;
      dk[h] = known - m[h];
      dm[h] = mean - m[h];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const unsigned at = (rg * R + j) * g.wu + q;
      Vec<4> o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o.v[k] = rows[j].v[k] + dk[k >> 1];
      o.store(g.x_out, at);
      if (g.xmean_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[k] = rows[j].v[k] + dm[k >> 1];
        o.store(g.xmean_out, at);
      }
    }
  }
}

// The mean of the block whose first element is x[at], rows W apart: the order of the 16-byte path.
template <int R>
__device__ __forceinline__ float block_mean_scalar(const float* x, unsigned at, unsigned W) {
  float c[R];
#pragma unroll
  for (int k = 0; k < R; ++k) c[k] = x[at + k];
  for (int j = 1; j < R; ++j) {
#pragma unroll
    for (int k = 0; k < R; ++k) c[k] += x[at + j * W + k];
  }
  return tree_sum<R>(c) * (1.f / (R * R));
}

// Scalar path: item i is block bx of row group rg; g.wu = W / r.
template <int R>
__global__ __launch_bounds__(256) void superres_scalar_kernel(unsigned total, Args g) {
  const unsigned stride = gridDim.x * 256, W = g.wu * R;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned rg = i / g.wu, bx = i - rg * g.wu, at = rg * R * W + bx * R, n = rg / g.hb / g.C;
    const float m = block_mean_scalar<R>(g.x, at, W);
    const float mean = g.a[n] * g.low[i];
    const float known = g.z ? mean + g.s[n] * (1.f / R) * g.z[i] : mean;
    const float dk = known - m, dm = mean - m;
    for (int j = 0; j < R; ++j) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const unsigned e = at + j * W + k;
        const float v = g.x[e];
        g.x_out[e] = v + dk;
        if (g.xmean_out) g.xmean_out[e] = v + dm;
      }
    }
  }
}

template <int R>
__global__ __launch_bounds__(256) void block_mean_vec_kernel(unsigned total, const float* x, float* out, unsigned wq) {
  const unsigned stride = gridDim.x * 256;
  for (unsigned base = blockIdx.x * 256; base < total; base += stride) {
    const unsigned i = base + threadIdx.x;
    const bool live = i < total;
    Vec<4> rows[R];
    unsigned rg, q;
    load_quad<R>(x, i, live, wq, rows, rg, q);
    float m[2];
    quad_means<R>(rows, m);
    if (!live) continue;
    if constexpr (R == 2) reinterpret_cast<float2*>(out)[rg * wq + q] = make_float2(m[0], m[1]);
    else if (q % (R / 4) == 0) out[rg * (wq / (R / 4)) + q / (R / 4)] = m[0];
  }
}

template <int R>
__global__ __launch_bounds__(256) void block_mean_scalar_kernel(unsigned total, const float* x, float* out, unsigned wb) {
  const unsigned stride = gridDim.x * 256, W = wb * R;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const unsigned rg = i / wb, bx = i - rg * wb;
    out[i] = block_mean_scalar<R>(x, rg * R * W + bx * R, W);
  }
}

// r in {2, 4, 8, 16}, H and W multiples of r, planes * H * W below 2^31.
bool supported(long planes, int H, int W, int r) {
  if (r != 2 && r != 4 && r != 8 && r != 16) return false;
  if (H % r || W % r) return false;
  const long LIMIT = 1L << 31;
  return planes < LIMIT && planes * H < LIMIT && planes * H * W < LIMIT;
}

template <int R>
int launch_superres(bool vec, const Args& g, unsigned total, hipStream_t st) {
  return stk_launch_vec(vec, superres_vec_kernel<R>, superres_scalar_kernel<R>, dim3(stk_ew_grid(total)), st, total, g);
}

template <int R>
int launch_block_mean(bool vec, const float* x, float* out, unsigned total, unsigned wu, hipStream_t st) {
  return stk_launch_vec(vec, block_mean_vec_kernel<R>, block_mean_scalar_kernel<R>, dim3(stk_ew_grid(total)), st, total, x, out,
                        wu);
}

}  // namespace

extern "C" int stk_superres_f32(const float* x, const float* low, const float* z, const float* a, const float* s, float* x_out,
                                float* xmean_out, int N, int C, int H, int W, int r, void* stream) {
  if (!x || !low || !a || !s || !x_out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return STK_EINVAL;
  if (!supported((long)N * C, H, W, r)) return STK_EUNSUPPORTED;
  const bool vec = (W & 3) == 0 && stk_all_aligned16(x, low, x_out, z, xmean_out);
  const unsigned hb = (unsigned)(H / r), wu = (unsigned)(vec ? W >> 2 : W / r);
  const unsigned total = (unsigned)N * (unsigned)C * hb * wu;
  const Args g{x, low, z, a, s, x_out, xmean_out, (unsigned)C, hb, wu};
  hipStream_t st = (hipStream_t)stream;
  switch (r) {
    case 2: return launch_superres<2>(vec, g, total, st);
    case 4: return launch_superres<4>(vec, g, total, st);
    case 8: return launch_superres<8>(vec, g, total, st);
    default: return launch_superres<16>(vec, g, total, st);
  }
}

extern "C" int stk_block_mean_f32(const float* x, float* out, long NC, int H, int W, int r, void* stream) {
  if (!x || !out || NC <= 0 || H <= 0 || W <= 0) return STK_EINVAL;
  if (!supported(NC, H, W, r)) return STK_EUNSUPPORTED;
  const bool vec = (W & 3) == 0 && stk_all_aligned16(x, out);
  const unsigned wu = (unsigned)(vec ? W >> 2 : W / r);
  const unsigned total = (unsigned)NC * (unsigned)(H / r) * wu;
  hipStream_t st = (hipStream_t)stream;
  switch (r) {
    case 2: return launch_block_mean<2>(vec, x, out, total, wu, st);
    case 4: return launch_block_mean<4>(vec, x, out, total, wu, st);
    case 8: return launch_block_mean<8>(vec, x, out, total, wu, st);
    default: return launch_block_mean<16>(vec, x, out, total, wu, st);
  }
}
