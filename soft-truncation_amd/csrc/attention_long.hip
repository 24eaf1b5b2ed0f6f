// attention_long.hip -- the attention core of AttnBlockpp on maps above 16 x 16 (include/stk_attention_long.h): the same
// quantities as attention.hip, for T up to 16384, with the long side streamed in chunks instead of held whole.
//
//   FWD  a workgroup owns 16 NW queries (16 per wave) and streams the keys in chunks of 32:  S^T = K^T Q (channels),
//        online softmax per query column (running maximum m and sum l; the o accumulator and l are multiplied by
//        exp(m_old - m_new) once per chunk, never deferred), o += V P^T;  o = acc / l,  lse = m + log l.
//   DQ   owns queries, streams keys:  S^T, dP^T = V^T dO;  p = exp(scale s - lse),  ds = p (dp - delta);  dq += K ds^T.
//   DKV  owns keys, streams queries:  S, dP = dO^T V;  p, ds as above;  dv += dO p,  dk += Q ds.
//   delta[t] = sum_c dO[c, t] o[c, t] comes from a pass of its own before DQ / DKV (it needs the forward's o).
// Every output element has one owning wave; nothing crosses workgroups, so two runs are bit-identical.
//
// Arithmetic (attention.hip): an operand tensor is multiplied by the power of two that puts its largest
// magnitude in [2^13, 2^14) and split into hi + lo fp16 planes; a product is lo hi + hi lo + hi hi, three
// v_mfma_f32_16x16x32_f16 with fp32 accumulation.  The planes are written ONCE per call into the caller's workspace (a
// per-workgroup conversion of all of K and V would repeat it T / 64 times per image) in the two layouts the MFMA fragments
// read without a transpose:
//   CF  "channel fast"   [plane][b][t][c]   an MFMA fragment wants 8 consecutive channels of one position (contractions
//                                           over channels: the scores and their gradient dP)
//   PF  "position fast"  [plane][b][c][t]   4 + 4 positions of one channel (contractions over positions: o, dq, dk, dv)
// with T padded to Tp = a multiple of 128 by zeros.  Probabilities (p <= 1) use the fixed scale 2^13.  The score gradient
// ds is scaled per owned column (query for DQ, key for DKV): the scale of a column is the power of two of the largest
// |ds| seen so far in it; when a chunk raises that maximum the scale drops and the column's accumulator is multiplied by
// the exact power-of-two ratio of the two scales.  Chunks with smaller |ds| keep the current scale (their terms land
// below 2^13 in the planes, exact to the fp16 subnormal step: 2^-37 of the column's largest term).  A chunk whose |ds|
// are all subnormal sets no scale; the epilogue undoes the tensor's and the column's scale one after the other, because
// their product may pass 2^127 where neither does (include/stk_attention_long.h, "Range").
//
// Fragment layouts of v_mfma_f32_16x16x32_f16 (lane l, r = l % 16, g = l / 16): A[i = r][k = 8 g + j], B[k = 8 g + j][n = r],
// D[i = 4 g + e][n = r].  A score tile of 32 streamed positions is two 16-row D tiles; lane (r, g) holds rows
// {4 g + e, 16 + 4 g + e} of column r, and these 8 values ARE its B fragment of the next contraction (k order permuted
// consistently: the A operand reads the same 4 + 4 positions from a PF row).  So p and ds never leave the registers.
#include "attention_mh.h"
#include "common.h"
#include "split.h"
#include "stk_attention_long.h"
#include "stk_attention_mh.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

constexpr int NPART = 256;       // partial |x| maxima per tensor (a scale record)
constexpr int KC = 32;           // streamed positions per chunk
constexpr int TPAD = 128;        // Tp: positions padded to a multiple of this (every kernel's tile divides it)
constexpr int PFP = 80;          // LDS pitch of a PF row: 32 positions (64 bytes) + 16
constexpr int TMAX = 16384;
constexpr float P_SCALE = 8192.f;  // probabilities are <= 1: 2^13

inline long tpad(int T) { return ((long)T + TPAD - 1) / TPAD * TPAD; }
// workspace regions (bytes each: both planes of one tensor in one layout)
enum { R_QCF, R_KCF, R_VPF, R_QPF, R_KPF, R_VCF, R_DCF, R_DPF, R_COUNT };
inline long region_bytes(int B, int C, int T) { return 2L * 2L * B * C * tpad(T); }

// ---- |x| maxima of up to four [B, C, T] tensors in one launch (blockIdx.y: the tensor) -------------------------------------
struct AmaxArgs { const float* x[4]; float* rec[4]; long bs4[4]; long ct4; long n4; };
__global__ __launch_bounds__(1024) void amax_kernel(AmaxArgs a) {
  __shared__ float red[16];
  const float4* x4 = reinterpret_cast<const float4*>(a.x[blockIdx.y]);
  const long bs4 = a.bs4[blockIdx.y], ct4 = a.ct4;
  float m = 0.f;
  for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < a.n4; i += (long)NPART * 1024) {
    const long b = i / ct4;
    const float4 u = x4[b * bs4 + (i - b * ct4)];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(u.x), fabsf(u.y))), fmaxf(fabsf(u.z), fabsf(u.w)));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < 16; ++w) m = fmaxf(m, red[w]);
    a.rec[blockIdx.y][blockIdx.x] = m;
  }
}

using split2::pow2_scale_of;      // the split rule itself: split.h
// scale of a tensor from its 256-entry record, computed by every wave on its own
__device__ __forceinline__ float rec_scale(const float* rec, int lane) {
  float m = fmaxf(fmaxf(rec[lane], rec[lane + 64]), fmaxf(rec[lane + 128], rec[lane + 192]));
  return pow2_scale_of(wave_max(m));
}

// ---- fp32 [B, C, T] (image stride bs) -> hi / lo fp16 planes, CF and / or PF layout -------------------------------------------
// grid (Tp / 64, C / 32, B), 256 threads: a tile of 32 channels x 64 positions; positions T .. Tp - 1 become zeros.
// Heads (include/stk_attention_mh.h): with D = C / heads < C the CF planes are written head-major, [plane][b][head][t][D],
// which is what the attention kernels read as B heads "images" of D channels; the PF layout [b][C][Tp] already is
// [b][head][D][Tp] (head n starts n D / 32 of these 32-channel blocks in).
struct SplitArgs { const float* x; long bs; const float* rec; _Float16* cf; _Float16* pf; long pe; int C, T, Tp, D; };
__global__ __launch_bounds__(256) void split_kernel(SplitArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 sh[2][64][32 + 8];
  const int tid = threadIdx.x, lane = tid & 63;
  const float s = rec_scale(a.rec, lane);
  const int b = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 64;
  const int t4 = (tid & 15) * 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int cc = (tid >> 4) + 16 * h, c = c0 + cc, t = p0 + t4;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < a.T) u = *reinterpret_cast<const float4*>(a.x + (long)b * a.bs + (long)c * a.T + t);
    const float v[4] = {s * u.x, s * u.y, s * u.z, s * u.w};
    halfx4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hi[i] = (_Float16)v[i];
      lo[i] = (_Float16)(v[i] - (float)hi[i]);
      sh[0][t4 + i][cc] = hi[i];
      sh[1][t4 + i][cc] = lo[i];
    }
    if (a.pf) {
      const long o = ((long)b * a.C + c) * a.Tp + t;
      *reinterpret_cast<halfx4*>(a.pf + o) = hi;
      *reinterpret_cast<halfx4*>(a.pf + a.pe + o) = lo;
    }
  }
  if (!a.cf) return;
  __syncthreads();
  const int tl = tid >> 2, part = tid & 3;
  const int hd = c0 / a.D;                                         // a 32-channel block lies in one head (D % 32 == 0)
  const long o = (((long)b * (a.C / a.D) + hd) * a.Tp + p0 + tl) * a.D + (c0 - hd * a.D) + part * 8;
#pragma unroll
  for (int p = 0; p < 2; ++p)
    *reinterpret_cast<halfx8*>(a.cf + p * a.pe + o) = *reinterpret_cast<const halfx8*>(&sh[p][tl][part * 8]);
}

// delta[b, t] = sum_c d_o[b, c, t] o[b, c, t]   (both contiguous [B, C, T]); grid (ceil(T / 256), B)
__global__ __launch_bounds__(256) void delta_kernel(const float* o, const float* d_o, float* delta, int C, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const long base = (long)b * C * T + t;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s = __fmaf_rn(d_o[base + (long)c * T], o[base + (long)c * T], s);
  delta[(long)b * T + t] = s;
}

// ---- helpers of the attention kernels ------------------------------------------------------------------------------------------
__device__ __forceinline__ void mma3(floatx4& acc, const halfx8& ah, const halfx8& al, const halfx8& bh, const halfx8& bl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);     // cross terms first (fixed order)
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}
__device__ __forceinline__ void split8(const float (&v)[8], halfx8& hi, halfx8& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hi[i] = (_Float16)v[i];
    lo[i] = (_Float16)(v[i] - (float)hi[i]);
  }
}
__device__ __forceinline__ halfx8 cat8(halfx4 a, halfx4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

// Stage one chunk of a CF tensor (rows j0 .. j0 + 31, all C channels, both planes) into LDS [plane][row][C] with pitch
// 2 C + 16 bytes, or of a PF tensor (all C channels, positions j0 .. j0 + 31) into [plane][c][32] with pitch PFP.  All
// loads of a call are issued before its stores.
template <int C, int NT>
__device__ __forceinline__ void stage_cf(unsigned char* dst, const _Float16* src, long pe, int b, int Tp, int j0, int tid) {
  constexpr int PR = C / 8, N = 2 * KC * PR, IT = (N + NT - 1) / NT, CFP = 2 * C + 16;
  uint4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int f = tid + i * NT;
    if (N % NT == 0 || f < N) {
      const int p = f / (KC * PR), rem = f - p * (KC * PR), row = rem / PR, col = rem - row * PR;
      v[i] = *reinterpret_cast<const uint4*>(src + p * pe + ((long)b * Tp + j0 + row) * C + col * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int f = tid + i * NT;
    if (N % NT == 0 || f < N) {
      const int p = f / (KC * PR), rem = f - p * (KC * PR), row = rem / PR, col = rem - row * PR;
      *reinterpret_cast<uint4*>(dst + p * KC * CFP + row * CFP + col * 16) = v[i];
    }
  }
}
template <int C, int NT>
__device__ __forceinline__ void stage_pf(unsigned char* dst, const _Float16* src, long pe, int b, int Tp, int j0, int tid) {
  constexpr int N = 2 * C * 4, IT = (N + NT - 1) / NT;
  uint4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int f = tid + i * NT;
    if (N % NT == 0 || f < N) {
      const int p = f / (C * 4), rem = f - p * C * 4, c = rem >> 2, part = rem & 3;
      v[i] = *reinterpret_cast<const uint4*>(src + p * pe + ((long)b * C + c) * Tp + j0 + part * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int f = tid + i * NT;
    if (N % NT == 0 || f < N) {
      const int p = f / (C * 4), rem = f - p * C * 4, c = rem >> 2, part = rem & 3;
      *reinterpret_cast<uint4*>(dst + p * C * PFP + c * PFP + part * 16) = v[i];
    }
  }
}
// A fragment (rows = streamed positions 16 u + r, channels 32 ks + 8 g ..) of a staged CF chunk, plane p
template <int C>
__device__ __forceinline__ halfx8 frag_cf(const unsigned char* t, int p, int u, int ks, int r, int g) {
  constexpr int CFP = 2 * C + 16;
  return *reinterpret_cast<const halfx8*>(t + p * KC * CFP + (16 * u + r) * CFP + (32 * ks + 8 * g) * 2);
}
// A fragment (rows = channels 16 cb + r, positions 4 g .. + 3 and 16 + 4 g .. + 3) of a staged PF chunk, plane p
template <int C>
__device__ __forceinline__ halfx8 frag_pf(const unsigned char* t, int p, int cb, int r, int g) {
  const unsigned char* row = t + p * C * PFP + (16 * cb + r) * PFP + 8 * g;
  return cat8(*reinterpret_cast<const halfx4*>(row), *reinterpret_cast<const halfx4*>(row + 32));
}
// B fragments (8 consecutive channels of one owned position, all C) of a CF tensor in global memory
template <int C>
__device__ __forceinline__ void own_frags(halfx8 (&h)[C / 32], halfx8 (&l)[C / 32], const _Float16* src, long pe, long row, int g) {
#pragma unroll
  for (int ks = 0; ks < C / 32; ++ks) {
    h[ks] = *reinterpret_cast<const halfx8*>(src + row * C + 32 * ks + 8 * g);
    l[ks] = *reinterpret_cast<const halfx8*>(src + pe + row * C + 32 * ks + 8 * g);
  }
}
// the per-column ds scale (see the head of the file): max |ds| of the chunk -> scale in use, accumulators rescaled
template <int NCB>
__device__ __forceinline__ void ds_rescale(float dmax, float& sig, floatx4 (&acc)[NCB]) {
  dmax = fmaxf(dmax, __shfl_xor(dmax, 16, 64));
  dmax = fmaxf(dmax, __shfl_xor(dmax, 32, 64));
  if (dmax >= 1.17549435e-38f) {                                   // a subnormal maximum sets no scale: pow2_scale_of gives 1,
    const float sc = pow2_scale_of(dmax);                          // which would pin the column's scale (it only drops)
    if (sig == 0.f || sc < sig) {
      if (sig != 0.f) {
        const float f = sc / sig;                                 // a power of two <= 1/2: exact
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] *= f;
      }
      sig = sc;
    }
  }
}

struct Planes { const _Float16* r[R_COUNT]; long pe; };         // hi plane of each region; lo = hi + pe
struct KArgs {
  Planes pl;
  float* out[2]; long os; float beta[2];                          // FWD: o;  DQ: dq;  DKV: dk, dv
  const float* rec;                                               // scale records q, k, v, d_o
  float* lse; const float* delta;
  int B, C, T, Tp; float scale;
  int H;                                                          // heads: B counts (image, head) pairs and C is one head's
};                                                                // width; pair b writes out at (b / H) os + (b % H) C T

template <int C, int NW>
__global__ __launch_bounds__(NW * 64) void fwd_kernel(KArgs a) {
  constexpr int NT = NW * 64, CFP = 2 * C + 16, NKS = C / 32, NCB = C / 16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KC * CFP + 2 * C * PFP];
  unsigned char* const kt = lds;
  unsigned char* const vt = lds + 2 * KC * CFP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T = a.T, Tp = a.Tp, ntile = Tp / (16 * NW);
  const int id = xcd_remap(blockIdx.x, gridDim.x), b = id / ntile;
  const int t = (id - b * ntile) * 16 * NW + 16 * w + r;          // the query of this lane's column
  const long pe = a.pl.pe;
  const float sq = rec_scale(a.rec, lane), sk = rec_scale(a.rec + NPART, lane), sv = rec_scale(a.rec + 2 * NPART, lane);
  const float us = a.scale / (sq * sk);
  halfx8 qh[NKS], ql[NKS];
  own_frags<C>(qh, ql, a.pl.r[R_QCF], pe, (long)b * Tp + t, g);
  floatx4 o[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) o[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                                   // l: this lane's part of the column sum

  for (int j0 = 0; j0 < T; j0 += KC) {
    __syncthreads();
    stage_cf<C, NT>(kt, a.pl.r[R_KCF], pe, b, Tp, j0, tid);
    stage_pf<C, NT>(vt, a.pl.r[R_VPF], pe, b, Tp, j0, tid);
    __syncthreads();
    floatx4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) mma3(s[u], frag_cf<C>(kt, 0, u, ks, r, g), frag_cf<C>(kt, 1, u, ks, r, g), qh[ks], ql[ks]);
    float x[8], mc = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int tk = j0 + 16 * (i >> 2) + 4 * g + (i & 3);
      x[i] = tk < T ? us * s[i >> 2][i & 3] : -INFINITY;
      mc = fmaxf(mc, x[i]);
    }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    const float mn = fmaxf(m, mc);                                 // finite: every chunk holds a key < T
    const float alpha = expf(m - mn);                              // 0 at the first chunk (m = -inf)
    float p[8], ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      p[i] = expf(x[i] - mn);
      ps += p[i];
      p[i] *= P_SCALE;
    }
    l = __fmaf_rn(l, alpha, ps);
    m = mn;
    halfx8 ph, pl;
    split8(p, ph, pl);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      o[cb] *= alpha;                                              // everything at the old maximum, exactly once
      mma3(o[cb], frag_pf<C>(vt, 0, cb, r, g), frag_pf<C>(vt, 1, cb, r, g), ph, pl);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (t < T) {
    const float inv = 1.f / (sv * P_SCALE * l);
    float* ob = a.out[0] + (long)(b / a.H) * a.os + (long)(b % a.H) * C * T + t;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[(long)(16 * cb + 4 * g + e) * T] = inv * o[cb][e];
    if (g == 0) a.lse[(long)b * T + t] = m + logf(l);
  }
}

template <int C, int NW>
__global__ __launch_bounds__(NW * 64) void dq_kernel(KArgs a) {
  constexpr int NT = NW * 64, CFP = 2 * C + 16, NKS = C / 32, NCB = C / 16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KC * CFP + 2 * C * PFP];
  unsigned char* const kc = lds;
  unsigned char* const vc = lds + 2 * KC * CFP;
  unsigned char* const kp = lds + 4 * KC * CFP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T = a.T, Tp = a.Tp, ntile = Tp / (16 * NW);
  const int id = xcd_remap(blockIdx.x, gridDim.x), b = id / ntile;
  const int t = (id - b * ntile) * 16 * NW + 16 * w + r;          // the query of this lane's column
  const long pe = a.pl.pe;
  const float sq = rec_scale(a.rec, lane), sk = rec_scale(a.rec + NPART, lane), sv = rec_scale(a.rec + 2 * NPART, lane),
              sd = rec_scale(a.rec + 3 * NPART, lane);
  const float us = a.scale / (sq * sk), ud = 1.f / (sv * sd);
  halfx8 qh[NKS], ql[NKS], dh[NKS], dl[NKS];
  own_frags<C>(qh, ql, a.pl.r[R_QCF], pe, (long)b * Tp + t, g);
  own_frags<C>(dh, dl, a.pl.r[R_DCF], pe, (long)b * Tp + t, g);
  const bool live = t < T;
  const float lse = live ? a.lse[(long)b * T + t] : 0.f, de = live ? a.delta[(long)b * T + t] : 0.f;
  floatx4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
  float sig = 0.f;                                                 // scale of this column's ds (0: none yet)

  for (int j0 = 0; j0 < T; j0 += KC) {
    __syncthreads();
    stage_cf<C, NT>(kc, a.pl.r[R_KCF], pe, b, Tp, j0, tid);
    stage_cf<C, NT>(vc, a.pl.r[R_VCF], pe, b, Tp, j0, tid);
    stage_pf<C, NT>(kp, a.pl.r[R_KPF], pe, b, Tp, j0, tid);
    __syncthreads();
    floatx4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, dp[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        mma3(s[u], frag_cf<C>(kc, 0, u, ks, r, g), frag_cf<C>(kc, 1, u, ks, r, g), qh[ks], ql[ks]);
        mma3(dp[u], frag_cf<C>(vc, 0, u, ks, r, g), frag_cf<C>(vc, 1, u, ks, r, g), dh[ks], dl[ks]);
      }
    float ds[8], dmax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int tk = j0 + 16 * (i >> 2) + 4 * g + (i & 3);
      const float p = (live && tk < T) ? expf(us * s[i >> 2][i & 3] - lse) : 0.f;
      ds[i] = p * (ud * dp[i >> 2][i & 3] - de);
      dmax = fmaxf(dmax, fabsf(ds[i]));
    }
    ds_rescale<NCB>(dmax, sig, acc);
    const float use = sig == 0.f ? 1.f : sig;
#pragma unroll
    for (int i = 0; i < 8; ++i) ds[i] *= use;
    halfx8 bh, bl;
    split8(ds, bh, bl);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) mma3(acc[cb], frag_pf<C>(kp, 0, cb, r, g), frag_pf<C>(kp, 1, cb, r, g), bh, bl);
  }
  if (live) {
    const float f = sig == 0.f ? 0.f : (a.scale / sk) / sig, beta = a.beta[0];   // not scale / (sk sig): sk sig may pass 2^127
    float* ob = a.out[0] + (long)(b / a.H) * a.os + (long)(b % a.H) * C * T + t;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float* d = ob + (long)(16 * cb + 4 * g + e) * T;
        const float v = f * acc[cb][e];
        *d = beta != 0.f ? __fmaf_rn(beta, *d, v) : v;
      }
  }
}

template <int C, int NW>
__global__ __launch_bounds__(NW * 64) void dkv_kernel(KArgs a) {
  constexpr int NT = NW * 64, CFP = 2 * C + 16, NKS = C / 32, NCB = C / 16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KC * CFP + 4 * C * PFP];
  unsigned char* const qc = lds;
  unsigned char* const dc = lds + 2 * KC * CFP;
  unsigned char* const qp = lds + 4 * KC * CFP;
  unsigned char* const dpf = lds + 4 * KC * CFP + 2 * C * PFP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T = a.T, Tp = a.Tp, ntile = Tp / (16 * NW);
  const int id = xcd_remap(blockIdx.x, gridDim.x), b = id / ntile;
  const int t = (id - b * ntile) * 16 * NW + 16 * w + r;          // the key of this lane's column
  const long pe = a.pl.pe;
  const float sq = rec_scale(a.rec, lane), sk = rec_scale(a.rec + NPART, lane), sv = rec_scale(a.rec + 2 * NPART, lane),
              sd = rec_scale(a.rec + 3 * NPART, lane);
  const float us = a.scale / (sq * sk), ud = 1.f / (sv * sd);
  halfx8 kh[NKS], kl[NKS], vh[NKS], vl[NKS];
  own_frags<C>(kh, kl, a.pl.r[R_KCF], pe, (long)b * Tp + t, g);
  own_frags<C>(vh, vl, a.pl.r[R_VCF], pe, (long)b * Tp + t, g);
  const bool live = t < T;
  floatx4 dk[NCB], dv[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) dk[cb] = dv[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
  float sig = 0.f;

  for (int j0 = 0; j0 < T; j0 += KC) {
    __syncthreads();
    stage_cf<C, NT>(qc, a.pl.r[R_QCF], pe, b, Tp, j0, tid);
    stage_cf<C, NT>(dc, a.pl.r[R_DCF], pe, b, Tp, j0, tid);
    stage_pf<C, NT>(qp, a.pl.r[R_QPF], pe, b, Tp, j0, tid);
    stage_pf<C, NT>(dpf, a.pl.r[R_DPF], pe, b, Tp, j0, tid);
    __syncthreads();
    floatx4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, dp[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        mma3(s[u], frag_cf<C>(qc, 0, u, ks, r, g), frag_cf<C>(qc, 1, u, ks, r, g), kh[ks], kl[ks]);
        mma3(dp[u], frag_cf<C>(dc, 0, u, ks, r, g), frag_cf<C>(dc, 1, u, ks, r, g), vh[ks], vl[ks]);
      }
    float p[8], ds[8], dmax = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tq = j0 + 16 * u + 4 * g;                          // rows tq .. tq + 3: whole inside or outside [0, T)
      float4 ls = make_float4(0.f, 0.f, 0.f, 0.f), dl = ls;
      if (tq < T) {
        ls = *reinterpret_cast<const float4*>(a.lse + (long)b * T + tq);
        dl = *reinterpret_cast<const float4*>(a.delta + (long)b * T + tq);
      }
      const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * u + e;
        const float pv = (live && tq < T) ? expf(us * s[u][e] - lsv[e]) : 0.f;
        ds[i] = pv * (ud * dp[u][e] - dlv[e]);
        p[i] = P_SCALE * pv;
        dmax = fmaxf(dmax, fabsf(ds[i]));
      }
    }
    halfx8 bh, bl;
    split8(p, bh, bl);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) mma3(dv[cb], frag_pf<C>(dpf, 0, cb, r, g), frag_pf<C>(dpf, 1, cb, r, g), bh, bl);
    ds_rescale<NCB>(dmax, sig, dk);
    const float use = sig == 0.f ? 1.f : sig;
#pragma unroll
    for (int i = 0; i < 8; ++i) ds[i] *= use;
    split8(ds, bh, bl);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) mma3(dk[cb], frag_pf<C>(qp, 0, cb, r, g), frag_pf<C>(qp, 1, cb, r, g), bh, bl);
  }
  if (live) {
    const float fk = sig == 0.f ? 0.f : (a.scale / sq) / sig, fv = 1.f / (sd * P_SCALE);   // as in dq_kernel
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      float* base = a.out[which];
      if (!base) continue;
      const float beta = a.beta[which], f = which == 0 ? fk : fv;
      float* ob = base + (long)(b / a.H) * a.os + (long)(b % a.H) * C * T + t;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float* d = ob + (long)(16 * cb + 4 * g + e) * T;
          const float v = f * (which == 0 ? dk[cb][e] : dv[cb][e]);
          *d = beta != 0.f ? __fmaf_rn(beta, *d, v) : v;
        }
    }
  }
}

// waves per workgroup: 8 where the owned operands and the accumulator leave room for two waves per SIMD, 4 for DKV (two
// owned operands and two accumulators) and for DQ from C = 224 on (which would spill at 256 registers)
constexpr int NW_FWD = 8, NW_DKV = 4;
template <int C> constexpr int nw_dq() { return C >= 224 ? 4 : 8; }

template <int MODE, int C>
void launch_c(const KArgs& a, hipStream_t s) {
  if (MODE == 0) hipLaunchKernelGGL((fwd_kernel<C, NW_FWD>), dim3(a.B * (a.Tp / (16 * NW_FWD))), dim3(NW_FWD * 64), 0, s, a);
  constexpr int NW_DQ = nw_dq<C>();
  if (MODE == 1) hipLaunchKernelGGL((dq_kernel<C, NW_DQ>), dim3(a.B * (a.Tp / (16 * NW_DQ))), dim3(NW_DQ * 64), 0, s, a);
  if (MODE == 2) hipLaunchKernelGGL((dkv_kernel<C, NW_DKV>), dim3(a.B * (a.Tp / (16 * NW_DKV))), dim3(NW_DKV * 64), 0, s, a);
}
template <int MODE>
int launch(const KArgs& a, hipStream_t s) {
  switch (a.C) {
    case 32: launch_c<MODE, 32>(a, s); break;
    case 64: launch_c<MODE, 64>(a, s); break;
    case 96: launch_c<MODE, 96>(a, s); break;
    case 128: launch_c<MODE, 128>(a, s); break;
    case 160: launch_c<MODE, 160>(a, s); break;
    case 192: launch_c<MODE, 192>(a, s); break;
    case 224: launch_c<MODE, 224>(a, s); break;
    case 256: launch_c<MODE, 256>(a, s); break;
    default: return STK_EUNSUPPORTED;
  }
  STK_CHECK_LAUNCH();
  return STK_OK;
}

// D = C / heads channels of one head (0: heads does not divide C); one head is the whole image
inline int mh_d(int C, int heads) { return heads > 0 && C > 0 && C % heads == 0 ? C / heads : 0; }
inline bool long_ok(int B, int C, int T, int heads = 1) {
  const int d = mh_d(C, heads);
  return B > 0 && d >= 32 && d <= 256 && d % 32 == 0 && T >= 4 && T <= TMAX && T % 4 == 0 && (long)B * C * T < 0x7fffffffL;
}
inline bool stride_ok(int B, int C, int T, long bs) {
  return bs >= (long)C * T && bs % 4 == 0 && (long)(B - 1) * bs + (long)C * T < 0x7fffffffL;
}
inline long ws_need(int B, int C, int T) { return R_COUNT * region_bytes(B, C, T); }
// what the entries refuse as unsupported once their pointers and sizes are valid (ws_bytes: the entry's own check)
inline bool fwd_operands_ok(const float* q, const float* k, const float* v, long bs, const void* ws, int B, int C, int T) {
  return stride_ok(B, C, T, bs) && stk_aligned16(q) && stk_aligned16(k) && stk_aligned16(v) && stk_aligned16(ws);
}
inline bool bwd_operands_ok(const float* q, const float* k, const float* v, long bs, const float* d_o, const float* lse,
                            const float* delta, long gs, const void* ws, int B, int C, int T) {
  return fwd_operands_ok(q, k, v, bs, ws, B, C, T) && stride_ok(B, C, T, gs) && stk_aligned16(d_o) && stk_aligned16(lse) &&
         stk_aligned16(delta);
}

Planes planes_of(void* ws, int B, int C, int T) {
  Planes p;
  const long rb = region_bytes(B, C, T);
  for (int i = 0; i < R_COUNT; ++i) p.r[i] = reinterpret_cast<const _Float16*>(static_cast<char*>(ws) + i * rb);
  p.pe = rb / 4;                                                   // halves per plane
  return p;
}
// |x| maxima of n [B, C, T] tensors of image stride bs into the records rec, rec + NPART, ...
int amax(const float* const* x, int n, long bs, float* rec, int B, int C, int T, hipStream_t s) {
  AmaxArgs m = {};
  for (int i = 0; i < n; ++i) { m.x[i] = x[i]; m.rec[i] = rec + i * NPART; m.bs4[i] = bs / 4; }
  m.ct4 = (long)C * T / 4; m.n4 = (long)B * m.ct4;
  hipLaunchKernelGGL(amax_kernel, dim3(NPART, n), dim3(1024), 0, s, m);
  STK_CHECK_LAUNCH();
  return STK_OK;
}
int split(const float* x, long bs, const float* rec, const Planes& pl, int cf, int pf, int B, int C, int T, int heads,
          hipStream_t s) {
  SplitArgs a;
  a.x = x; a.bs = bs; a.rec = rec; a.pe = pl.pe; a.C = C; a.T = T; a.Tp = (int)tpad(T); a.D = C / heads;
  a.cf = cf < 0 ? nullptr : const_cast<_Float16*>(pl.r[cf]);
  a.pf = pf < 0 ? nullptr : const_cast<_Float16*>(pl.r[pf]);
  hipLaunchKernelGGL(split_kernel, dim3(a.Tp / 64, C / 32, B), dim3(256), 0, s, a);
  STK_CHECK_LAUNCH();
  return STK_OK;
}
void base_args(KArgs& a, const Planes& pl, const float* rec, int B, int C, int T, float scale, int heads) {
  a.pl = pl; a.rec = rec; a.B = B * heads; a.C = C / heads; a.T = T; a.Tp = (int)tpad(T); a.scale = scale; a.H = heads;
}

// The one streaming body of each direction, behind the checks of the entries below.  With heads > 1 the kernels above run
// unchanged on B heads pairs of D = C / heads channels: the planes are split from the whole tensors (one scale per tensor),
// head-major where the layout is channel-fast, and only the address of an output tile knows that a pair is a slice of an
// image.  delta's [B, heads, T] rows are those of [B heads, D, T] tensors.
int long_fwd(const float* q, const float* k, const float* v, long bs, float* o, float* lse, float* rec, int B, int C, int T,
             int heads, float scale, void* ws, hipStream_t s) {
  const float* qkv[3] = {q, k, v};
  int rc;
  if ((rc = amax(qkv, 3, bs, rec, B, C, T, s))) return rc;
  const Planes pl = planes_of(ws, B, C, T);
  if ((rc = split(q, bs, rec, pl, R_QCF, -1, B, C, T, heads, s))) return rc;
  if ((rc = split(k, bs, rec + NPART, pl, R_KCF, -1, B, C, T, heads, s))) return rc;
  if ((rc = split(v, bs, rec + 2 * NPART, pl, -1, R_VPF, B, C, T, heads, s))) return rc;
  KArgs a = {};
  base_args(a, pl, rec, B, C, T, scale, heads);
  a.out[0] = o; a.os = (long)C * T; a.lse = lse;
  return launch<0>(a, s);
}

int long_bwd(const float* q, const float* k, const float* v, long bs, const float* o, const float* d_o, const float* lse,
             float* rec, float* delta, float* dq, float beta_q, float* dk, float beta_k, float* dv, float beta_v, long gs,
             int B, int C, int T, int heads, float scale, void* ws, hipStream_t s) {
  const long ct = (long)C * T;
  float* rdo = rec + 3 * NPART;
  int rc;
  if ((rc = amax(&d_o, 1, ct, rdo, B, C, T, s))) return rc;
  hipLaunchKernelGGL(delta_kernel, dim3((T + 255) / 256, B * heads), dim3(256), 0, s, o, d_o, delta, C / heads, T);
  STK_CHECK_LAUNCH();
  const Planes pl = planes_of(ws, B, C, T);
  if ((rc = split(q, bs, rec, pl, R_QCF, R_QPF, B, C, T, heads, s))) return rc;
  if ((rc = split(k, bs, rec + NPART, pl, R_KCF, R_KPF, B, C, T, heads, s))) return rc;
  if ((rc = split(v, bs, rec + 2 * NPART, pl, R_VCF, -1, B, C, T, heads, s))) return rc;
  if ((rc = split(d_o, ct, rdo, pl, R_DCF, R_DPF, B, C, T, heads, s))) return rc;
  KArgs a = {};
  base_args(a, pl, rec, B, C, T, scale, heads);
  a.lse = const_cast<float*>(lse); a.delta = delta; a.os = gs;
  if (dq) {
    a.out[0] = dq; a.beta[0] = beta_q;
    if ((rc = launch<1>(a, s))) return rc;
  }
  if (dk || dv) {
    a.out[0] = dk; a.beta[0] = beta_k; a.out[1] = dv; a.beta[1] = beta_v;
    if ((rc = launch<2>(a, s))) return rc;
  }
  return STK_OK;
}

inline bool mh_short(int T) { return T <= 256; }   // include/stk_attention_mh.h: the short form (attention.hip) up to here

}  // namespace

extern "C" {

// ---- include/stk_attention_long.h -------------------------------------------------------------------------------------------
int stk_attention_long_ok(int B, int C, int T) { return long_ok(B, C, T) ? 1 : 0; }

long stk_attention_long_ws_bytes(int B, int C, int T) { return long_ok(B, C, T) ? ws_need(B, C, T) : STK_EUNSUPPORTED; }

int stk_attention_long_fwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, float* o, float* lse,
                               float* rec, int B, int C, int T, float scale, void* ws, long ws_bytes, void* stream) {
  if (!q || !k || !v || !o || !lse || !rec || !ws || B <= 0 || C <= 0 || T <= 0) return STK_EINVAL;
  if (!long_ok(B, C, T) || !fwd_operands_ok(q, k, v, qkv_bstride, ws, B, C, T) || ws_bytes < ws_need(B, C, T))
    return STK_EUNSUPPORTED;
  return long_fwd(q, k, v, qkv_bstride, o, lse, rec, B, C, T, 1, scale, ws, (hipStream_t)stream);
}

int stk_attention_long_bwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, const float* o,
                               const float* d_o, const float* lse, float* rec, float* delta, float* dq, float beta_q,
                               float* dk, float beta_k, float* dv, float beta_v, long grad_bstride, int B, int C, int T,
                               float scale, void* ws, long ws_bytes, void* stream) {
  if (!q || !k || !v || !o || !d_o || !lse || !rec || !delta || !ws || B <= 0 || C <= 0 || T <= 0) return STK_EINVAL;
  if (!long_ok(B, C, T) || !bwd_operands_ok(q, k, v, qkv_bstride, d_o, lse, delta, grad_bstride, ws, B, C, T) ||
      ws_bytes < ws_need(B, C, T))
    return STK_EUNSUPPORTED;
  return long_bwd(q, k, v, qkv_bstride, o, d_o, lse, rec, delta, dq, beta_q, dk, beta_k, dv, beta_v, grad_bstride, B, C, T, 1,
                  scale, ws, (hipStream_t)stream);
}

// ---- include/stk_attention_mh.h: the short form (attention.hip, through attention_mh.h) or the streaming one, by T ------------
int stk_attention_mh_ok(int B, int C, int T, int heads) {
  return (mh_short(T) ? stk_mh::short_ok(B, C, T, heads) : long_ok(B, C, T, heads)) ? 1 : 0;
}

long stk_attention_mh_ws_bytes(int B, int C, int T, int heads) {
  if (B <= 0 || C <= 0 || T <= 0 || heads <= 0 || C % heads) return STK_EINVAL;
  if (!stk_attention_mh_ok(B, C, T, heads)) return STK_EUNSUPPORTED;
  return mh_short(T) ? 0 : ws_need(B, C, T);
}

int stk_attention_mh_fwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, float* o, float* lse,
                             float* rec, int B, int C, int T, int heads, float scale, void* ws, long ws_bytes,
                             void* stream) {
  if (!q || !k || !v || !o || !lse || !rec || B <= 0 || C <= 0 || T <= 0 || heads <= 0 || C % heads) return STK_EINVAL;
  if (!stk_attention_mh_ok(B, C, T, heads)) return STK_EUNSUPPORTED;
  if (mh_short(T)) return stk_mh::short_fwd(q, k, v, qkv_bstride, o, lse, rec, B, C, T, heads, scale, stream);
  if (!ws || ws_bytes < ws_need(B, C, T)) return STK_EINVAL;
  if (!fwd_operands_ok(q, k, v, qkv_bstride, ws, B, C, T)) return STK_EUNSUPPORTED;
  return long_fwd(q, k, v, qkv_bstride, o, lse, rec, B, C, T, heads, scale, ws, (hipStream_t)stream);
}

int stk_attention_mh_bwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, const float* o,
                             const float* d_o, const float* lse, float* rec, float* delta, float* dq, float beta_q,
                             float* dk, float beta_k, float* dv, float beta_v, long grad_bstride, int B, int C, int T,
                             int heads, float scale, void* ws, long ws_bytes, void* stream) {
  if (!q || !k || !v || !o || !d_o || !lse || !rec || !delta || B <= 0 || C <= 0 || T <= 0 || heads <= 0 || C % heads)
    return STK_EINVAL;
  if (!stk_attention_mh_ok(B, C, T, heads)) return STK_EUNSUPPORTED;
  if (mh_short(T))
    return stk_mh::short_bwd(q, k, v, qkv_bstride, d_o, lse, rec, delta, dq, beta_q, dk, beta_k, dv, beta_v, grad_bstride, B, C,
                             T, heads, scale, stream);
  if (!ws || ws_bytes < ws_need(B, C, T)) return STK_EINVAL;
  if (!bwd_operands_ok(q, k, v, qkv_bstride, d_o, lse, delta, grad_bstride, ws, B, C, T)) return STK_EUNSUPPORTED;
  return long_bwd(q, k, v, qkv_bstride, o, d_o, lse, rec, delta, dq, beta_q, dk, beta_k, dv, beta_v, grad_bstride, B, C, T,
                  heads, scale, ws, (hipStream_t)stream);
}

}  // extern "C"
