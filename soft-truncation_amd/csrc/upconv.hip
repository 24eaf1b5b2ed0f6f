// upconv.hip -- the FIR-upsampling convolution (include/stk_upconv.h) on the fp32 MFMA core (igemm.h), for gfx950.
//
// out = FIR(u),  u = conv_transpose(x, w) at stride 2 = the correlation of w with x zero-stuffed to (2H-1) x (2W-1).
// The stuffed map is never formed and none of its zeros is multiplied:
//
//   forward   one GEMM per output parity (py, px) of u.  Row oy = 2a + py meets a sample only through the taps
//             kh = py + 2s (K is odd), at input row i = a + s + py - (K-1)/2:
//                 M = Cout   N = batch * PH * PW   K = Cin * ty * tx   A = w[:, :, py::2, px::2]   B = shifted x
//             with ty = (K+1)/2 taps on the even rows and (K-1)/2 on the odd ones: 4 + 2 + 2 + 1 = 9 products per input
//             pixel and channel pair for K = 3, against 36 for the stuffed form.  The epilogue scatters the tile into its
//             parity of u (a stride-2 store); the FIR kernel below then reads u once and applies bias / res / out_div.
//   dgrad     M = Cin   N = batch * H * W   K = Cout * K * K   A = w^T (taps reversed)   B = du[2i + kh', 2j + kw']:
//             a dense stride-2 gather, every element in range (u is 2H-2+K wide), no holes.
//   wgrad     M = Cout  N = Cin   K = batch * H * W, one GEMM per tap, A = du[2i + (K-1) - kh, 2j + (K-1) - kw], B = x,
//             split over the pixels into slabs [tap][Cout][Cin] that a second kernel sums in a fixed order into dw.
//
// Tiles: igemm's 128 x 128 (64 x 64 where that leaves CUs idle) with 32-deep k chunks (36 = 4 channels x 9 taps for the
// 3x3 data gradient), v_mfma_f32_32x32x2_f32, k-major LDS tiles with an odd pitch.  Loaders follow conv.hip's rules:
// unconditional loads from safe addresses, validity in a bitmask applied at the LDS store.
#include "igemm.h"
#include "stk_upconv.h"

namespace {

using igemm::Cfg;
using igemm::MnMajor;
using igemm::keep_if;
using igemm::strip_row;

typedef __attribute__((address_space(1))) float gfloat;

struct UpP {
  const float* x; const float* w; const float* du;     // du: the map u (forward: written, gradients: read)
  float* u; float* dx; float beta, alpha;
  float* part; long part_stride;
  int N, H, W, Cin, Cout, K, KK, half;                  // half = (K-1)/2
  int UH, UW, HW, UHW;
  int py, px, ty, tx, PH, PW, PHW;                      // forward: this launch's parity, its taps and its output grid
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// A(m=co, k=(ci, s, t)) = w[co, ci, py + 2s, px + 2t]: lanes walk k (a thread keeps one k of the 32-chunk and NA rows), so a
// half-wave reads the taps of 8 / 16 / 32 consecutive channels of one row: a few cache lines per load.
template <class C, int TAPS>
struct AUpFwd {
  static_assert(C::KC == 32 && C::NA <= 32, "32-deep chunks");
  int roff[C::NA]; int tid; unsigned okrows, okm;
  __device__ void init(const UpP& p, int m0, int tid_, int) {
    tid = tid_; okrows = 0; okm = 0;
#pragma unroll
    for (int i = 0; i < C::NA; ++i) {
      const int m = m0 + (tid >> 5) + 8 * i;
      okrows |= (m < p.Cout ? 1u : 0u) << i;
      roff[i] = min(m, p.Cout - 1) * p.Cin * p.KK;
    }
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NA]) {
    const int k = k0 + (tid & 31);
    const int ci = k / TAPS, tap = k % TAPS;
    const int sy = tap / p.tx, sx = tap - sy * p.tx;
    const bool ok = ci < p.Cin;
    const int off = ok ? ci * p.KK + (p.py + 2 * sy) * p.K + p.px + 2 * sx : 0;
    okm = ok ? okrows : 0u;
#pragma unroll
    for (int i = 0; i < C::NA; ++i) r[i] = p.w[roff[i] + off];
  }
  __device__ void store(const float (&r)[C::NA], float* t) {
#pragma unroll
    for (int i = 0; i < C::NA; ++i) t[(tid & 31) * C::LDA + (tid >> 5) + 8 * i] = keep_if(r[i], okm, i);
  }
};

// B(k=(ci, s, t), n=(b, a, c)) = x[b, ci, a + s + py - half, c + t + px - half], zero outside the map; lanes along pixels.
template <class C, int TAPS>
struct BUpFwd {
  using Mp = MnMajor<C::BN, C::KC>;
  static constexpr int NCH = C::NB / TAPS;
  static_assert(Mp::PER % TAPS == 0 && C::NB <= 32, "k rows per thread must cover whole channels");
  int tb, cig, tid; int toff[TAPS]; unsigned mask, okm;
  __device__ void init(const UpP& p, int n0, int tid_, int) {
    tid = tid_;
    const int n = n0 + Mp::mn(tid);
    cig = __builtin_amdgcn_readfirstlane(Mp::kgroup(tid) * (Mp::PER / TAPS));
    mask = 0; okm = 0; tb = 0;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) toff[t] = (t / p.tx) * p.W + (t % p.tx);
    if (n < p.N * p.PHW) {
      const int b = n / p.PHW, r = n - b * p.PHW;
      const int a = r / p.PW, c = r - a * p.PW;
      const int iy0 = a + p.py - p.half, ix0 = c + p.px - p.half;
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const int iy = iy0 + t / p.tx, ix = ix0 + t % p.tx;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) mask |= 1u << t;
      }
      tb = b * p.Cin * p.HW + iy0 * p.W + ix0;
    }
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NB]) {
    const int ci0 = k0 / TAPS + cig;          // scalar
    okm = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ci = ci0 + c;
      const unsigned cm = ci < p.Cin ? mask : 0u;
      okm |= cm << (c * TAPS);
      const int cs = min(ci, p.Cin - 1);
      const gfloat* plane = (const gfloat*)((uintptr_t)p.x + (uintptr_t)cs * (uintptr_t)p.HW * 4u);
#pragma unroll
      for (int t = 0; t < TAPS; ++t) r[c * TAPS + t] = plane[((cm >> t) & 1u) ? tb + toff[t] : 0];
    }
  }
  __device__ void store(const float (&r)[C::NB], float* t) {
    const int kg = Mp::kgroup(tid) * Mp::PER, mn = Mp::mn(tid);
#pragma unroll
    for (int i = 0; i < C::NB; ++i) t[(kg + i) * C::LDB + mn] = keep_if(r[i], okm, i);
  }
};

struct EpUpFwd {      // u[b, co, 2a + py, 2c + px] = acc
  int col_off;
  __device__ void init(const UpP&, int, int) {}
  __device__ void col(const UpP& p, int n) {
    const int b = n / p.PHW, r = n - b * p.PHW;
    const int a = r / p.PW, c = r - a * p.PW;
    col_off = b * p.Cout * p.UHW + (2 * a + p.py) * p.UW + 2 * c + p.px;
  }
  __device__ void strip(const UpP& p, int mbase, int M, bool nok, int, const floatx16& acc) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = mbase + strip_row(e);
      if (nok && m < M) p.u[col_off + m * p.UHW] = acc[e];
    }
  }
};

// ---- data gradient -----------------------------------------------------------------------------------------------------
// 3x3: A(m=ci, k=(co, t')) = w[co, ci, 8 - t']: the nine taps of a (co, ci) pair are contiguous -> 4 threads per row, one co
// each, nine loads at immediate offsets, stored to LDS in reversed order.
template <class C>
struct AUpDg9 {
  static_assert(C::KC == 36, "3x3 chunks are 4 channels x 9 taps");
  static constexpr int PASSES = C::BM / 64;
  int m0, tid; unsigned okp;
  __device__ void init(const UpP&, int m0_, int tid_, int) { m0 = m0_; tid = tid_; okp = 0; }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NA]) {
    const int co = k0 / 9 + (tid & 3);
    okp = 0;
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int m = m0 + (tid >> 2) + 64 * ps;
      const bool ok = m < p.Cin && co < p.Cout;
      const float* s = p.w + (ok ? ((long)co * p.Cin + m) * 9 : 0);
#pragma unroll
      for (int j = 0; j < 9; ++j) r[ps * 9 + j] = s[8 - j];
      okp |= (ok ? 1u : 0u) << ps;
    }
  }
  __device__ void store(const float (&r)[C::NA], float* t) {
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps)
#pragma unroll
      for (int j = 0; j < 9; ++j)
        t[((tid & 3) * 9 + j) * C::LDA + (tid >> 2) + 64 * ps] = keep_if(r[ps * 9 + j], okp, ps);
  }
};
// 1x1: A(m=ci, k=co) = w[co, ci]  (m contiguous: lanes along m)
template <class C>
struct AUpDg1 {
  using Mp = MnMajor<C::BM, C::KC>;
  int tid, kg; const float* pm; bool ok; unsigned okm;
  __device__ void init(const UpP& p, int m0, int tid_, int) {
    tid = tid_; okm = 0;
    const int m = m0 + Mp::mn(tid);
    ok = m < p.Cin;
    pm = p.w + (ok ? m : 0);
    kg = Mp::kgroup(tid) * Mp::PER;
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NA]) {
    okm = 0;
#pragma unroll
    for (int i = 0; i < Mp::PER; ++i) {
      const int k = k0 + kg + i;
      const bool v = ok && k < p.Cout;
      r[i] = pm[v ? (long)k * p.Cin : 0];
      okm |= (v ? 1u : 0u) << i;
    }
  }
  __device__ void store(const float (&r)[C::NA], float* t) {
#pragma unroll
    for (int i = 0; i < Mp::PER; ++i) t[(kg + i) * C::LDA + Mp::mn(tid)] = keep_if(r[i], okm, i);
  }
};
// B(k=(co, t'), n=(b, i, j)) = du[b, co, 2i + t'/K, 2j + t'%K]: always inside the map
template <class C, int TAPS>
struct BUpDg {
  using Mp = MnMajor<C::BN, C::KC>;
  static constexpr int NCH = C::NB / TAPS;
  static_assert(Mp::PER % TAPS == 0 && C::NB <= 32, "k rows per thread must cover whole channels");
  int tb, cig, tid; bool ok; unsigned okm;
  __device__ void init(const UpP& p, int n0, int tid_, int) {
    tid = tid_;
    const int n = n0 + Mp::mn(tid);
    cig = __builtin_amdgcn_readfirstlane(Mp::kgroup(tid) * (Mp::PER / TAPS));
    okm = 0; tb = 0;
    ok = n < p.N * p.HW;
    if (ok) {
      const int b = n / p.HW, hw = n - b * p.HW;
      const int i = hw / p.W, j = hw - i * p.W;
      tb = b * p.Cout * p.UHW + 2 * i * p.UW + 2 * j;
    }
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NB]) {
    const int co0 = k0 / TAPS + cig;          // scalar
    constexpr int KW = TAPS == 9 ? 3 : 1;
    okm = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int co = co0 + c;
      const bool v = ok && co < p.Cout;
      const int cb = v ? tb + co * p.UHW : 0;
      okm |= (v ? ((1u << TAPS) - 1u) : 0u) << (c * TAPS);
#pragma unroll
      for (int t = 0; t < TAPS; ++t) r[c * TAPS + t] = p.du[v ? cb + (t / KW) * p.UW + (t % KW) : 0];
    }
  }
  __device__ void store(const float (&r)[C::NB], float* t) {
    const int kg = Mp::kgroup(tid) * Mp::PER, mn = Mp::mn(tid);
#pragma unroll
    for (int i = 0; i < C::NB; ++i) t[(kg + i) * C::LDB + mn] = keep_if(r[i], okm, i);
  }
};
struct EpUpDg {       // dx = beta dx + alpha acc
  int col_off;
  __device__ void init(const UpP&, int, int) {}
  __device__ void col(const UpP& p, int n) {
    const int b = n / p.HW;
    col_off = b * p.Cin * p.HW + (n - b * p.HW);
  }
  __device__ void strip(const UpP& p, int mbase, int M, bool nok, int, const floatx16& acc) {
#pragma unroll
    for (int e0 = 0; e0 < 16; e0 += 4) {
      float old[4]; int idx[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = mbase + strip_row(e0 + q);
        idx[q] = (nok && m < M) ? col_off + m * p.HW : -1;
        old[q] = (p.beta != 0.f && idx[q] >= 0) ? p.beta * p.dx[idx[q]] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (idx[q] >= 0) p.dx[idx[q]] = old[q] + p.alpha * acc[e0 + q];
    }
  }
};

// ---- weight gradient (K = pixels of x, lanes along pixels; tap = zb) -----------------------------------------------------
__device__ __forceinline__ void up_pixel(const UpP& p, int k, int& b, int& hw, int& i, int& j) {
  b = k / p.HW; hw = k - b * p.HW;
  i = hw / p.W; j = hw - i * p.W;
}
template <class C>
struct AUpWg {        // A(m=co, k=(b, i, j)) = du[b, co, 2i + (K-1) - kh, 2j + (K-1) - kw]
  static_assert(C::KC == 32 && C::NA <= 32, "32-pixel chunks");
  int roff[C::NA]; int tid, dy, dx; unsigned okrows, okm;
  __device__ void init(const UpP& p, int m0, int tid_, int zb) {
    tid = tid_; okm = 0; okrows = 0;
    const int kh = zb / p.K, kw = zb - kh * p.K;
    dy = p.K - 1 - kh; dx = p.K - 1 - kw;
#pragma unroll
    for (int i = 0; i < C::NA; ++i) {
      const int m = m0 + (tid >> 5) + 8 * i;
      okrows |= (m < p.Cout ? 1u : 0u) << i;
      roff[i] = min(m, p.Cout - 1) * p.UHW;
    }
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NA]) {
    const int k = k0 + (tid & 31);
    const bool kv = k < p.N * p.HW;
    int b, hw, i, j;
    up_pixel(p, kv ? k : 0, b, hw, i, j);
    const int base = b * p.Cout * p.UHW + (2 * i + dy) * p.UW + 2 * j + dx;
    okm = kv ? okrows : 0u;
#pragma unroll
    for (int q = 0; q < C::NA; ++q) r[q] = p.du[base + roff[q]];
  }
  __device__ void store(const float (&r)[C::NA], float* t) {
#pragma unroll
    for (int i = 0; i < C::NA; ++i) t[(tid & 31) * C::LDA + (tid >> 5) + 8 * i] = keep_if(r[i], okm, i);
  }
};
template <class C>
struct BUpWg {        // B(k=(b, i, j), n=ci) = x[b, ci, i, j]
  static_assert(C::KC == 32 && C::NB <= 32, "32-pixel chunks");
  int roff[C::NB]; int tid; unsigned okrows, okm;
  __device__ void init(const UpP& p, int n0, int tid_, int) {
    tid = tid_; okm = 0; okrows = 0;
#pragma unroll
    for (int i = 0; i < C::NB; ++i) {
      const int ci = n0 + (tid >> 5) + 8 * i;
      okrows |= (ci < p.Cin ? 1u : 0u) << i;
      roff[i] = min(ci, p.Cin - 1) * p.HW;
    }
  }
  __device__ void load(const UpP& p, int k0, float (&r)[C::NB]) {
    const int k = k0 + (tid & 31);
    const bool kv = k < p.N * p.HW;
    const int ks = kv ? k : 0;
    const int b = ks / p.HW, hw = ks - b * p.HW;
    const int base = b * p.Cin * p.HW + hw;
    okm = kv ? okrows : 0u;
#pragma unroll
    for (int q = 0; q < C::NB; ++q) r[q] = p.x[base + roff[q]];
  }
  __device__ void store(const float (&r)[C::NB], float* t) {
#pragma unroll
    for (int i = 0; i < C::NB; ++i) t[(tid & 31) * C::LDB + (tid >> 5) + 8 * i] = keep_if(r[i], okm, i);
  }
};
struct EpUpWg {       // partial slab of split zs as [tap][Cout][Cin] (lanes = ci, contiguous)
  float* slab; int tap;
  __device__ void init(const UpP& p, int zb, int zs) { slab = p.part + (long)zs * p.part_stride; tap = zb; }
  __device__ void col(const UpP&, int) {}
  __device__ void strip(const UpP& p, int mbase, int M, bool nok, int n, const floatx16& acc) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = mbase + strip_row(e);
      if (nok && m < M) slab[((long)tap * p.Cout + m) * p.Cin + n] = acc[e];
    }
  }
};
// dw[co, ci, tap] += alpha * sum over the splits (z ascending: the result does not depend on the launch geometry) of
// slab[tap][co][ci].  Threads walk the slab order, so the `splits` reads per element are coalesced.
__global__ __launch_bounds__(256) void up_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long n,
                                                        int splits, long stride, float alpha, long CC, int taps) {
  const long gstride = (long)gridDim.x * 256;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += gstride) {
    float sum = 0.f;
    for (int z = 0; z < splits; ++z) sum += part[(long)z * stride + j];
    const int tap = (int)(j / CC);
    dw[(j - (long)tap * CC) * taps + tap] += alpha * sum;
  }
}

// ---- the FIR passes: 1:1, taps KT x KT, out[y, x] = sum_a,b T[a][b] in[y + a - oy0, x + b - ox0], in = 0 outside ------------
// forward: T = the flipped taps, oy0 = pad0, then (+ bias + res) / out_div; adjoint: T = the taps, oy0 = KT - 1 - pad0.
// A thread owns four consecutive outputs of a row: KT rows of KT + 3 loads feed 4 KT^2 multiply-adds.
template <int KT>
__global__ __launch_bounds__(256) void up_fir_kernel(const float* __restrict__ in, const float* __restrict__ taps,
                                                     float* __restrict__ out, long planes, int C, int IH, int IW, int OH,
                                                     int OW, int oy0, int ox0, int flip, const float* __restrict__ bias,
                                                     const float* __restrict__ res, float inv_div, int use_div) {
  float T[KT][KT];
#pragma unroll
  for (int a = 0; a < KT; ++a)
#pragma unroll
    for (int b = 0; b < KT; ++b) T[a][b] = flip ? taps[(KT - 1 - a) * KT + (KT - 1 - b)] : taps[a * KT + b];
  const int OWQ = (OW + 3) / 4;
  const long total = planes * OH * OWQ, gstride = (long)gridDim.x * 256;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += gstride) {
    const int xq = (int)(idx % OWQ);
    const long rest = idx / OWQ;
    const int y = (int)(rest % OH);
    const long pl = rest / OH;
    const int x0 = xq * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < KT; ++a) {
      const int iy = y + a - oy0;
      const bool rok = iy >= 0 && iy < IH;
      const float* row = in + (pl * IH + (rok ? iy : 0)) * IW;
      float v[KT + 3];
#pragma unroll
      for (int b = 0; b < KT + 3; ++b) {
        const int ix = x0 + b - ox0;
        const bool ok = rok && ix >= 0 && ix < IW;
        v[b] = ok ? row[ix] : 0.f;
      }
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int b = 0; b < KT; ++b) acc[o] = fmaf(T[a][b], v[o + b], acc[o]);
    }
    const long obase = (pl * OH + y) * OW + x0;
    const float bv = bias ? bias[(int)(pl % C)] : 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (x0 + o < OW) {
        float r = acc[o];
        if (bias) r += bv;
        if (res) r += res[obase + o];
        if (use_div) r *= inv_div;
        out[obase + o] = r;
      }
    }
  }
}

int launch_fir(const float* in, const float* taps, float* out, long planes, int C, int IH, int IW, int OH, int OW, int oy0,
               int ox0, int flip, const float* bias, const float* res, float out_div, int KT, hipStream_t s) {
  const long items = planes * OH * ((OW + 3) / 4);
  const dim3 grid((unsigned)stk_ew_grid(items)), block(256);
  const float inv = 1.f / out_div;
  const int use_div = out_div != 1.f;
#define UP_FIR(T) hipLaunchKernelGGL((up_fir_kernel<T>), grid, block, 0, s, in, taps, out, planes, C, IH, IW, OH, OW, oy0, ox0, \
                                     flip, bias, res, inv, use_div)
  switch (KT) {
    case 1: UP_FIR(1); break;
    case 2: UP_FIR(2); break;
    case 3: UP_FIR(3); break;
    case 4: UP_FIR(4); break;
    default: return STK_EUNSUPPORTED;
  }
#undef UP_FIR
  STK_CHECK_LAUNCH();
  return STK_OK;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline bool big_tile(int M, long N, int z) {      // conv.hip's rule: 128 x 128 tiles when they still give every CU work
  const long t = (long)stk_cdiv(M, 128) * stk_cdiv(N, 128) * z;
  return M >= 96 && N >= 96 && t >= 192;
}

template <class C, class AL, class BL, class EP>
int launch(const UpP& p, int M, long Nl, int K, int k_per_split, int splits, int batch, hipStream_t s, bool flat = false) {
  if (Nl > 0x7fffffffL) return STK_EUNSUPPORTED;
  const int N = (int)Nl;
  const int tm = stk_cdiv(M, C::BM), tn = stk_cdiv(N, C::BN);
  if (flat) {
    const long total = (long)tm * tn * splits * batch;
    if (total > 0x7fffffffL) return STK_EUNSUPPORTED;
    hipLaunchKernelGGL((igemm::kernel<C, UpP, AL, BL, EP>), dim3((unsigned)total), dim3(256), 0, s, p, M, N, K, tm, tn,
                       k_per_split, batch);
  } else {
    hipLaunchKernelGGL((igemm::kernel<C, UpP, AL, BL, EP>), dim3((unsigned)(tm * tn), (unsigned)splits, (unsigned)batch),
                       dim3(256), 0, s, p, M, N, K, tm, tn, k_per_split, 0);
  }
  STK_CHECK_LAUNCH();
  return STK_OK;
}

int fill(UpP& p, int N, int H, int W, int Cin, int Cout, int K, int KT) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return STK_EINVAL;
  if ((K != 1 && K != 3) || KT < 1 || KT > 4) return STK_EUNSUPPORTED;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = K; p.KK = K * K; p.half = (K - 1) / 2;
  p.UH = 2 * H - 2 + K; p.UW = 2 * W - 2 + K; p.HW = H * W; p.UHW = p.UH * p.UW;
  const long lim = 0x7fffffffL;       // 32-bit element offsets inside the kernels
  if ((long)N * Cin * p.HW >= lim || (long)N * Cout * p.UHW >= lim || (long)N * Cout * 4 * p.HW >= lim ||
      (long)Cout * Cin * p.KK >= lim)
    return STK_EUNSUPPORTED;
  return STK_OK;
}

struct UpWgPlan { int big; int splits; int k_per_split; long slab; };
UpWgPlan wg_plan(const UpP& p) {      // conv.hip's per-tap plan: ~512 workgroups, >= 16 chunks of 32 pixels each
  UpWgPlan q;
  const long K = (long)p.N * p.HW;
  const long tiles128 = (long)stk_cdiv(p.Cout, 128) * stk_cdiv(p.Cin, 128) * p.KK;
  q.big = (p.Cout >= 96 && p.Cin >= 96 && tiles128 >= 9) ? 1 : 0;
  const int T = q.big ? 128 : 64;
  const long tiles = (long)stk_cdiv(p.Cout, T) * stk_cdiv(p.Cin, T) * p.KK;
  const long chunks = (K + 31) / 32;
  long splits = (512 + tiles - 1) / tiles;
  if (splits > chunks / 16) splits = chunks / 16;
  if (splits < 1) splits = 1;
  const long cps = (chunks + splits - 1) / splits;
  q.k_per_split = (int)(cps * 32);
  q.splits = (int)((K + q.k_per_split - 1) / q.k_per_split);
  q.slab = (long)p.Cout * p.Cin * p.KK;
  return q;
}

// one parity of the forward
template <int TAPS>
int launch_phase(const UpP& p, hipStream_t s) {
  using CB = Cfg<128, 128, 32>; using CS = Cfg<64, 64, 32>;
  const long Ng = (long)p.N * p.PHW;
  const int Kd = p.Cin * TAPS;
  if (big_tile(p.Cout, Ng, 1)) return launch<CB, AUpFwd<CB, TAPS>, BUpFwd<CB, TAPS>, EpUpFwd>(p, p.Cout, Ng, Kd, Kd, 1, 1, s);
  return launch<CS, AUpFwd<CS, TAPS>, BUpFwd<CS, TAPS>, EpUpFwd>(p, p.Cout, Ng, Kd, Kd, 1, 1, s);
}

// du = adjoint FIR of dy
int make_du(const UpP& p, const float* dy, const float* fir, float* du, int KT, int pad0, hipStream_t s) {
  return launch_fir(dy, fir, du, (long)p.N * p.Cout, p.Cout, 2 * p.H, 2 * p.W, p.UH, p.UW, KT - 1 - pad0, KT - 1 - pad0, 0,
                    nullptr, nullptr, 1.f, KT, s);
}

}  // namespace

extern "C" {

long stk_upconv2d_ws_bytes(int dir, int N, int H, int W, int Cin, int Cout, int K, int KT) {
  UpP p = {};
  if (fill(p, N, H, W, Cin, Cout, K, KT) != STK_OK || dir < 0 || dir > 2) return -1;
  if (dir == 0) return (long)N * Cout * p.UHW * 4;
  if (dir == 1) return 0;
  const UpWgPlan q = wg_plan(p);
  return (long)q.splits * q.slab * 4;
}

int stk_upconv2d_fwd_f32(const float* x, const float* w, const float* fir, const float* bias, const float* res,
                         float out_div, float* y, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0,
                         void* ws, long ws_bytes, void* stream) {
  if (!x || !w || !fir || !y || !ws || out_div == 0.f) return STK_EINVAL;
  UpP p = {};
  int rc = fill(p, N, H, W, Cin, Cout, K, KT);
  if (rc) return rc;
  if (ws_bytes < (long)N * Cout * p.UHW * 4) return STK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* u = reinterpret_cast<float*>(ws);
  p.x = x; p.w = w; p.u = u;
  if (K == 1) {
    // only the even-even parity of u meets a sample; the stuffed zeros of the other three are u itself here
    if (hipMemsetAsync(u, 0, (size_t)N * Cout * p.UHW * 4, s) != hipSuccess) return STK_ELAUNCH;
  }
  for (int py = 0; py < 2; ++py) {
    for (int px = 0; px < 2; ++px) {
      p.py = py; p.px = px;
      p.ty = py == 0 ? (K + 1) / 2 : (K - 1) / 2;
      p.tx = px == 0 ? (K + 1) / 2 : (K - 1) / 2;
      p.PH = py == 0 ? (p.UH + 1) / 2 : p.UH / 2;
      p.PW = px == 0 ? (p.UW + 1) / 2 : p.UW / 2;
      p.PHW = p.PH * p.PW;
      const int taps = p.ty * p.tx;
      if (taps == 0 || p.PHW == 0) continue;
      if (taps == 4) rc = launch_phase<4>(p, s);
      else if (taps == 2) rc = launch_phase<2>(p, s);
      else rc = launch_phase<1>(p, s);
      if (rc) return rc;
    }
  }
  return launch_fir(u, fir, y, (long)N * Cout, Cout, p.UH, p.UW, 2 * H, 2 * W, pad0, pad0, 1, bias, res, out_div, KT, s);
}

int stk_upconv2d_dgrad_f32(const float* dy, const float* w, const float* fir, float* du, int du_valid, float* dx,
                           float beta, float alpha, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0,
                           void* stream) {
  if (!w || !du || !dx || (!du_valid && (!dy || !fir))) return STK_EINVAL;
  UpP p = {};
  int rc = fill(p, N, H, W, Cin, Cout, K, KT);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!du_valid && (rc = make_du(p, dy, fir, du, KT, pad0, s))) return rc;
  p.w = w; p.du = du; p.dx = dx; p.beta = beta; p.alpha = alpha;
  const long Ng = (long)N * p.HW;
  const int Kd = Cout * p.KK;
  const bool big = big_tile(Cin, Ng, 1);
  if (K == 3) {
    using CB = Cfg<128, 128, 36>; using CS = Cfg<64, 64, 36>;
    if (big) return launch<CB, AUpDg9<CB>, BUpDg<CB, 9>, EpUpDg>(p, Cin, Ng, Kd, Kd, 1, 1, s);
    return launch<CS, AUpDg9<CS>, BUpDg<CS, 9>, EpUpDg>(p, Cin, Ng, Kd, Kd, 1, 1, s);
  }
  using CB = Cfg<128, 128, 32>; using CS = Cfg<64, 64, 32>;
  if (big) return launch<CB, AUpDg1<CB>, BUpDg<CB, 1>, EpUpDg>(p, Cin, Ng, Kd, Kd, 1, 1, s);
  return launch<CS, AUpDg1<CS>, BUpDg<CS, 1>, EpUpDg>(p, Cin, Ng, Kd, Kd, 1, 1, s);
}

int stk_upconv2d_wgrad_f32(const float* x, const float* dy, const float* fir, float* du, int du_valid, float* dw,
                           float alpha, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0, void* ws,
                           long ws_bytes, void* stream) {
  if (!x || !du || !dw || !ws || (!du_valid && (!dy || !fir))) return STK_EINVAL;
  UpP p = {};
  int rc = fill(p, N, H, W, Cin, Cout, K, KT);
  if (rc) return rc;
  const UpWgPlan q = wg_plan(p);
  if (ws_bytes < (long)q.splits * q.slab * 4) return STK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!du_valid && (rc = make_du(p, dy, fir, du, KT, pad0, s))) return rc;
  p.x = x; p.du = du; p.part = reinterpret_cast<float*>(ws); p.part_stride = q.slab;
  const long Kl = (long)N * p.HW;
  const int Kd = (int)Kl;
  using CB = Cfg<128, 128, 32>; using CS = Cfg<64, 64, 32>;
  if (q.big) rc = launch<CB, AUpWg<CB>, BUpWg<CB>, EpUpWg>(p, Cout, Cin, Kd, q.k_per_split, q.splits, p.KK, s, true);
  else rc = launch<CS, AUpWg<CS>, BUpWg<CS>, EpUpWg>(p, Cout, Cin, Kd, q.k_per_split, q.splits, p.KK, s, true);
  if (rc) return rc;
  hipLaunchKernelGGL(up_reduce_kernel, dim3(stk_ew_grid(q.slab)), dim3(256), 0, s, p.part, dw, q.slab, q.splits, q.slab, alpha,
                     (long)Cout * Cin, p.KK);
  STK_CHECK_LAUNCH();
  return STK_OK;
}

}  // extern "C"
