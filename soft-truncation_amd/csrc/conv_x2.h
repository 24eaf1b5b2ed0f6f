// conv_x2.h -- forward / data-gradient convolution (3x3 pad 1 and 1x1, stride 1) on the fp16 matrix pipe with a TWO-way
// operand split ("x2"), for gfx950, and what the split kernels share: tile geometry, the activation-operand descriptor (Src),
// raw buffer loads, the fp32 row loaders of the weight gradients and the sizing helpers.  Included by conv.hip inside its
// anonymous namespace; conv_pl.h, conv_x2d.h and conv_x2w.h follow it and build on namespace x2.
//
// Why: the split kernels are limited by the matrix pipe's power-limited clock, i.e. by the number of MFMAs.  An fp32
// value is, to 2^-24 relative, the sum of two fp16 values (11 + 11 significand bits, round to nearest), so
//     a*b = a0*b0 + (a0*b1 + a1*b0) + O(2^-22 |ab|)
// needs THREE fp16 MFMAs where a bf16 three-way split needs six (8 + 8 + 8 bits).  fp16 has only 5
// exponent bits, so each operand tensor is first multiplied by the power of two that puts its largest magnitude in
// [2^13, 2^14) -- exact, and undone exactly in the epilogue.  An element more than 2^-16 below its tensor's maximum
// loses (part of) its second term to fp16's subnormal range; its error then stays below 2^-39 of that maximum.
// Measured against float64 (tools/split_accuracy.py, bench.py `arithmetic_check`): 0.8-1.6e-6 of max|y|, the same as the
// f32-input MFMA and the bf16 three-way split, also for gradient-like tensors whose images spread over four decades.
//
// Scales: the weights' |w| maximum is taken when they are prepared (wamax -> 256-byte header of the prepared block); an
// activation tensor's |x| maximum comes from amax_partial_kernel, launched by the conv call itself: 256 partial maxima
// that every workgroup of the consumer reduces on its own, so there is no finishing launch and no host round trip.
//
// K is ordered (32-channel group, tap, channel in group): a 32-wide k chunk is one tap and 32 consecutive channels,
// so the tap (hence the halo test and the pixel shift) is uniform over the chunk and a thread's 16 loads differ only
// by a scalar channel-plane offset; and the nine chunks of a channel group follow each other, so the nine shifted
// reads of the same 32 x (128 + halo) activation patch hit L1 / L2.
#pragma once

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

namespace x2 {

using split2::pow2_scale_of;      // the split rule itself: split.h (included by conv.hip at file scope)
using split2::pack_h2;
using split2::lo_part;

constexpr int KC = 32;
constexpr int PITCH = 80;              // bytes per LDS row: 32 fp16 + 16 bytes of padding
constexpr int PLANE = 128 * PITCH;     // one split plane of one operand
constexpr int OPER = 2 * PLANE;
constexpr int LDS_BYTES = 2 * OPER;    // 40960
constexpr int NPART = 256;             // partial maxima per activation tensor
constexpr int HEADER = 256;            // bytes in front of the planes of a prepared block: WPART partial |w| maxima

struct Src {             // the activation operand: channel-concat of two NCHW tensors
  const float* s1; const float* s2; int S1, S2;
  const unsigned short* wp; int Mpad; int Kc;     // prepared weights, padded row count, channels (= S1 + S2)
  int taps;                                       // 9 (3x3, pad 1) or 1 (1x1)
  const unsigned char* pl; long pl_stride;        // pre-split activation planes (conv_pl.h) and bytes per plane, or null
};

// All global reads of the split kernels are raw BUFFER loads: a wave-uniform resource (tensor base + size in SGPRs), one
// 32-bit per-lane byte offset and a scalar offset per load, so a chunk's loads cost no per-load address VALU; and a read
// outside the tensor returns 0 instead of faulting, which is how halo lanes are zeroed (offset bit 31 set) and why
// a shifted 16-pixel run may start one element before / end one element after its tensor.
// (Buffer offsets are 32-bit: the host side keeps these kernels to tensors below 2 GB.)
// The wrappers themselves are common.h's (stk_make_rsrc, stk_buf_load), shared with the epilogues of conv.hip.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, long bytes) { return stk_make_rsrc(base, bytes); }
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) { return stk_buf_load(r, voff, soff); }

inline int pad128(int v) { return (v + 127) / 128 * 128; }

// part[b] = max |x| over block b's grid-stride share (any n; 16-byte path when aligned).  1024 threads per block and two
// independent 16-byte loads per thread and trip: with 256 x 256 threads the pass ran at 2.6 TB/s, latency-bound.
constexpr int AMAX_THREADS = 1024;
__global__ __launch_bounds__(AMAX_THREADS) void amax_partial_kernel(const float* __restrict__ x, long n,
                                                                   float* __restrict__ part) {
  __shared__ float red[AMAX_THREADS / 64];
  float m0 = 0.f, m1 = 0.f;
  const long n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n >> 2 : 0;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const long stride = (long)NPART * AMAX_THREADS;
  long i = (long)blockIdx.x * AMAX_THREADS + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const float4 u = x4[i], v = x4[i + stride];
    m0 = fmaxf(fmaxf(m0, fmaxf(fabsf(u.x), fabsf(u.y))), fmaxf(fabsf(u.z), fabsf(u.w)));
    m1 = fmaxf(fmaxf(m1, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (i < n4) {
    const float4 u = x4[i];
    m0 = fmaxf(fmaxf(m0, fmaxf(fabsf(u.x), fabsf(u.y))), fmaxf(fabsf(u.z), fabsf(u.w)));
  }
  for (long j = 4 * n4 + (long)blockIdx.x * AMAX_THREADS + threadIdx.x; j < n; j += stride) m1 = fmaxf(m1, fabsf(x[j]));
  float m = wave_max(fmaxf(m0, m1));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < AMAX_THREADS / 64; ++w) m = fmaxf(m, red[w]);
    part[blockIdx.x] = m;
  }
}

// block-wide maximum of `count` (256 or 512) partials; all 256 threads call it; `red` = 4 floats of LDS
__device__ __forceinline__ float block_amax(const float* __restrict__ part, int count, float* red) {
  float m = part[threadIdx.x];
  if (count > NPART) m = fmaxf(m, part[NPART + threadIdx.x]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return m;
}

// The same maximum with the LOADS at the top of a kernel and the reduction after its main loop (round 6): the scale of a plane operand
// is needed by the epilogue only, so its load latency (and the barriers of the reduction) need not stand in front of the first tile load --
// 2-3 us per workgroup round, which a 27 us K-split launch or a one-round weight gradient notices.  `red`: 4 floats of LDS of its own.
struct LateAmax {
  float m;
  __device__ __forceinline__ void load(const float* __restrict__ part, int count, int tid) {
    m = part[tid];
    if (count > NPART) m = fmaxf(m, part[NPART + tid]);
  }
  __device__ __forceinline__ float reduce(float* red, int tid) {            // all 256 threads of the (group of the) workgroup
    const float v = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
};

// ---- weight preparation ---------------------------------------------------------------------------------------------
// A prepared block = [HEADER bytes: partial |w| maxima][2 planes: Wp[split][k / 32][tap][row (pad 128)][k % 32] fp16 of scale*W],
// W(row, k, tap) = w[row * sm + k * sk + tap] (taps reversed when flip).  WprepDesc == StkWprepDesc (include/stk.h); wp points at the header.
struct WprepDesc {
  const float* w; unsigned char* wp; long sm, sk; int M, Kc, Mpad, taps, flip, reserved;
};
// |w| maxima: WPART workgroups per layer (blockIdx.y = layer, blockIdx.x = share) write one partial each into the header;
// the consumers (wprep_kernel, gemm_kernel) take the maximum of the WPART floats.  No atomics, nothing to zero.
constexpr int WPART = 16;
__global__ __launch_bounds__(256) void wamax_kernel(const WprepDesc* __restrict__ descs, WprepDesc one) {
  __shared__ float red[4];
  const WprepDesc d = descs ? descs[blockIdx.y] : one;
  const long n = (long)d.M * d.Kc * d.taps;
  float m = 0.f;
  if ((reinterpret_cast<uintptr_t>(d.w) & 15) == 0) {
    // 16-byte loads, four in flight per thread (round 4: one 4-byte load per trip made the 16 workgroups of a 256 x 256 x 9
    // layer walk 144 dependent round trips each -- 186 us per step for 232 MB)
    const float4* w4 = reinterpret_cast<const float4*>(d.w);
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < n4; i += (long)WPART * 1024) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long j = i + 256 * u;
        v[u] = j < n4 ? w4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(d.w[(n4 << 2) + threadIdx.x]));
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)WPART * 256) m = fmaxf(m, fabsf(d.w[i]));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) reinterpret_cast<float*>(d.wp)[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float weight_scale(const void* header) {
  const float* h = static_cast<const float*>(header);
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < WPART; ++i) m = fmaxf(m, h[i]);
  return pow2_scale_of(m);
}
// blockIdx.y picks the layer (or `one`), blockIdx.x walks its (row, k) pairs.  (Tried: a thread converting 8 consecutive k
// of a row for every tap and writing 16-byte pieces instead of 2-byte elements -- its strided reads made it 790 us per
// step against 340.)
__global__ __launch_bounds__(256) void wprep_kernel(const WprepDesc* __restrict__ descs, WprepDesc one) {
  const WprepDesc d = descs ? descs[blockIdx.y] : one;
  const long total = (long)d.Mpad * d.Kc;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float s = weight_scale(d.wp);
  unsigned short* out = reinterpret_cast<unsigned short*>(d.wp + HEADER);
  const int kl = (int)(i & 31);                      // k fastest inside a group of 32: contiguous 2-byte stores
  const long rest = i >> 5;
  const int row = (int)(rest % d.Mpad), cc = (int)(rest / d.Mpad), k = cc * 32 + kl;
  const long plane = (long)d.taps * d.Mpad * d.Kc;
  const float* src = d.w + (row < d.M ? row * d.sm + k * d.sk : 0);
  for (int t = 0; t < d.taps; ++t) {
    const float a = row < d.M ? s * src[d.flip ? d.taps - 1 - t : t] : 0.f;
    const _Float16 h0 = (_Float16)a, h1 = (_Float16)(a - (float)h0);
    const long o = (((long)cc * d.taps + t) * d.Mpad + row) * 32 + kl;
    out[o] = __builtin_bit_cast(unsigned short, h0);
    out[plane + o] = __builtin_bit_cast(unsigned short, h1);
  }
}
inline long wp_bytes(int M, int Kc, int taps) { return HEADER + 2L * taps * pad128(M) * Kc * 2; }

// ---- loaders ---------------------------------------------------------------------------------------------------------
// Staging is cut into slices so that a kernel can place slices between its MFMAs (the hipcc scheduler, left alone, runs
// the whole staging phase first and the MFMAs after it).  A loader provides
//     st(g, tile)        slice g of "registers of the current chunk -> LDS"
//     ld(g, ...)         slice g of "global -> registers for chunk c"
// and st(g) of a chunk always precedes ld(g) of the next one, so a register is reloaded only after its slice consumed it.
//
// 16 fp32 values of one LDS row -> two fp16 planes.  Slices 0..7 convert one pair each, 8..11 write one 16-byte piece.
// X1 (the one-product forward of include/stk_fp16.h): the hi plane only -- one rounding, no lo residual.
template <bool X1>
struct Split16X {
  unsigned pk[2][8];
  __device__ __forceinline__ void st(int g, const float (&r)[16], float s, unsigned char* tile, int row, int k0,
                                     unsigned okm = 0xffffu) {
    if (g < 8) {
      const float v0 = s * igemm::keep_if(r[2 * g], okm, 2 * g), v1 = s * igemm::keep_if(r[2 * g + 1], okm, 2 * g + 1);
      pk[0][g] = pack_h2(v0, v1);
      if (!X1) pk[1][g] = pack_h2(lo_part(v0), lo_part(v1));
    } else if (g < 12) {
      const int sp = (g - 8) >> 1, h = (g - 8) & 1;
      if (X1 && sp) return;
      *reinterpret_cast<u32x4*>(tile + sp * PLANE + row * PITCH + k0 * 2 + h * 16) =
          u32x4{pk[sp][4 * h], pk[sp][4 * h + 1], pk[sp][4 * h + 2], pk[sp][4 * h + 3]};
    }
  }
};
using Split16 = Split16X<false>;

struct WpLoader {        // four 16-byte pieces per chunk: split j>>1, row (tid>>2) + 64 (j&1), segment tid&3
  __amdgpu_buffer_rsrc_t rs; unsigned voff, plane2, chunk2; int row, seg;
  u32x4 r[4];
  __device__ __forceinline__ void init(const Src& q, int m0, int tid) {
    row = tid >> 2; seg = tid & 3;
    plane2 = (unsigned)q.taps * q.Mpad * q.Kc * 2u;
    chunk2 = (unsigned)q.Mpad * KC * 2u;
    rs = make_rsrc(reinterpret_cast<const unsigned char*>(q.wp) + HEADER, 2L * plane2);
    voff = ((unsigned)(m0 + row) * KC + seg * 8) * 2u;
  }
  __device__ __forceinline__ void ld(int g, int c) {
    if (g >= 4) return;
    r[g] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                         rs, (int)voff, (int)((unsigned)c * chunk2 + (g >> 1) * plane2 + (g & 1) * 64u * KC * 2u), 0));
  }
  __device__ __forceinline__ void st(int g, unsigned char* t) {
    if (g < 4) *reinterpret_cast<u32x4*>(t + (g >> 1) * PLANE + (row + 64 * (g & 1)) * PITCH + seg * 16) = r[g];
  }
};

// activations, lanes along pixels; a thread holds 16 channels of one tap-shifted pixel
template <bool DUAL, int TAPS, bool X1>
struct ActLoaderT {
  __amdgpu_buffer_rsrc_t rs1, rs2;
  int nl, kg, tb1, tb2; unsigned mask; float scale;
  float r[16]; Split16X<X1> sp;
  __device__ __forceinline__ void init(const ConvP& p, const Src& q, int n0, int tid, float s) {
    nl = tid & 127;
    kg = __builtin_amdgcn_readfirstlane(tid >> 7);      // which 16 of the chunk's 32 channels
    rs1 = make_rsrc(q.s1, (long)p.N * q.S1 * p.HW * 4);
    rs2 = make_rsrc(q.s2, (long)p.N * (DUAL ? q.S2 : q.S1) * p.HW * 4);
    mask = 0; tb1 = 0; tb2 = 0; scale = s;
    const int n = n0 + nl;
    if (n < p.N * p.HW) {
      const int b = n / p.HW, hw = n - b * p.HW;
      const int y = hw / p.W, x = hw - y * p.W;
      if (TAPS == 1) mask = 1u;
#pragma unroll
      for (int t = 0; t < (TAPS == 9 ? 9 : 0); ++t) {
        const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) mask |= 1u << t;
      }
      tb1 = b * q.S1 * p.HW + hw;
      tb2 = b * q.S2 * p.HW + hw;
    }
  }
  // slices 8..23 load one channel each (its register was consumed by conversion slice (g - 8) / 2 <= 7)
  __device__ __forceinline__ void ld(int g, const ConvP& p, const Src& q, int c) {
    if (g < 8) return;
    const int cc = TAPS == 9 ? c / 9 : c, tap = c - cc * TAPS;   // scalar: chunk = (32-channel group, tap), tap fastest
    const int ci0 = cc * KC + kg * 16;
    const bool first = !DUAL || ci0 < q.S1;                      // scalar: a chunk never straddles the two sources
    const __amdgpu_buffer_rsrc_t rs = first ? rs1 : rs2;
    const unsigned so = (unsigned)(first ? ci0 : ci0 - q.S1) * p.HW * 4u;
    const unsigned dead = (((mask >> tap) & 1u) ^ 1u) << 31;     // halo lanes: outside the buffer -> 0
    const int shift = TAPS == 9 ? (tap / 3 - 1) * p.W + (tap % 3 - 1) : 0;
    const unsigned vo = (unsigned)(((first ? tb1 : tb2) + shift) * 4) | dead;
    r[g - 8] = bload(rs, vo, so + (unsigned)(g - 8) * p.HW * 4u);
  }
  __device__ __forceinline__ void st(int g, unsigned char* t) { sp.st(g, r, scale, t, nl, kg * 16); }
};
template <bool DUAL, int TAPS> struct ActLoader : ActLoaderT<DUAL, TAPS, false> {};
template <bool DUAL, int TAPS> struct ActLoader16 : ActLoaderT<DUAL, TAPS, true> {};     // hi plane only (OneProduct forward)

// (Round 4, measured and dropped: a loader for the 1x1 layers that fetches 4 pixels x 4 channels per thread with 16-byte loads
// instead of 16 four-byte ones -- what had made the per-tap weight gradient 30 % faster -- changes nothing here: 384 -> 128 at
// 32 x 32 53.2 vs 52.3 us, 256 -> 256 data gradient 42.6 vs 41.3.  These kernels are not address-bound: a workgroup has 8-16
// chunks in all, and the chunk time is the staging round trip of the fp32-operand pipeline, profiles/r04_experiments.txt.)
// ---- the kernel: out tile 128 x 128, 4 waves of 64 x 64, chunks of 32 k; 12 MFMAs per 16-k step and wave -------------
// Grid (XCD-remapped): one flat dimension of tiles x K-splits.  xpart: `nxpart` (256 / 512) partial |x| maxima.
// X1 (EP = OneProduct<..>, include/stk_fp16.h): only the hi(w) hi(x) MFMAs of each half chunk (4 of 12) are issued, with an
// ActLoader16 (no lo plane) as BL.
template <class BL, class EP, int WPS = 2>       // WPS: waves per SIMD the register allocation must admit
__global__ __launch_bounds__(256, WPS) void gemm_kernel(ConvP p, Src q, int M, int Nn, int tiles_m, int tiles_n,
                                                   int nchunks_total, int chunks_per_split, const float* __restrict__ xpart,
                                                   int nxpart) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  constexpr bool X1 = is_x1<EP>::value;
  unsigned char* As = lds;
  unsigned char* Bs = lds + OPER;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const float sx = pow2_scale_of(block_amax(xpart, nxpart, reinterpret_cast<float*>(lds)));
  const float sw = weight_scale(q.wp);
  const float unscale = (1.f / sw) / sx;      // powers of two, one after the other (exact): sw sx may pass 2^127 (tiny operands)
  const int ntiles = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = id % ntiles, zs = id / ntiles;
  const int tm = tile % tiles_m, tn = tile / tiles_m;
  const int m0 = tm * 128, n0 = tn * 128;
  const int c_begin = zs * chunks_per_split;
  const int c_last = min(nchunks_total, c_begin + chunks_per_split) - 1;     // >= c_begin by construction

  WpLoader al; BL bl;
  al.init(q, m0, tid);
  bl.init(p, q, n0, tid, sx);
  EP ep;
  ep.preload(p, m0, n0, 128, M, Nn, tid);

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int wm0 = (wid & 1) * 64, wn0 = (wid >> 1) * 64;
  const int fk = lane >> 5, fc = lane & 31;
  const unsigned char* a_rd = As + (wm0 + fc) * PITCH + fk * 16;
  const unsigned char* b_rd = Bs + (wn0 + fc) * PITCH + fk * 16;

  // Pipeline: LDS single-buffered, two barriers per chunk.  Chunk c + 1 waits in registers while the first half of chunk c
  // is multiplied; behind the second half it goes to LDS and chunk c + 2's loads are issued -- each of those 12 MFMAs
  // carries TWO of the 24 staging slices.
#define STK_X2_FRAGS(KK)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int s = 0; s < 2; ++s) {         \
    a[i][s] = *reinterpret_cast<const halfx8*>(a_rd + s * PLANE + i * 32 * PITCH + (KK) * 32);          \
    b[i][s] = *reinterpret_cast<const halfx8*>(b_rd + s * PLANE + i * 32 * PITCH + (KK) * 32);          \
  }
  // three products per tile, the two cross terms first; MFMA g: product g / 4, tile (g / 2) & 1, g & 1
  constexpr int SA[3] = {1, 0, 0}, SB[3] = {0, 1, 0};
#define STK_X2_MFMA(G)                                                                                              \
  if (!X1 || ((G) >> 2) == 2)                                                                                       \
  acc[((G) >> 1) & 1][(G) & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[((G) >> 1) & 1][SA[(G) >> 2]], b[(G) & 1][SB[(G) >> 2]], \
                                                                        acc[((G) >> 1) & 1][(G) & 1], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 24; ++g) { al.ld(g, c_begin); bl.ld(g, p, q, c_begin); }
  {
    const int c1 = min(c_begin + 1, c_last);
#pragma unroll
    for (int g = 0; g < 24; ++g) { al.st(g, As); bl.st(g, Bs); al.ld(g, c1); bl.ld(g, p, q, c1); }
  }
  halfx8 a[2][2], b[2][2];
  for (int c = c_begin; c < c_last; ++c) {
    __syncthreads();                                   // B1: chunk c is in LDS
    STK_X2_FRAGS(0)
#pragma unroll
    for (int g = 0; g < 12; ++g) { STK_X2_MFMA(g) }
    STK_X2_FRAGS(1)
    __syncthreads();                                   // B2: nobody reads LDS any more
    const int c2 = min(c + 2, c_last);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < 12; ++g) {
      STK_X2_MFMA(g)
      al.st(2 * g, As); bl.st(2 * g, Bs); al.st(2 * g + 1, As); bl.st(2 * g + 1, Bs);      // chunk c + 1 -> LDS
      al.ld(2 * g, c2); bl.ld(2 * g, p, q, c2); al.ld(2 * g + 1, c2); bl.ld(2 * g + 1, p, q, c2);   // chunk c + 2
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();
  STK_X2_FRAGS(0)
#pragma unroll
  for (int g = 0; g < 12; ++g) { STK_X2_MFMA(g) }
  STK_X2_FRAGS(1)
#pragma unroll
  for (int g = 0; g < 12; ++g) { STK_X2_MFMA(g) }
#undef STK_X2_MFMA
#undef STK_X2_FRAGS

  ep.stage(lds, tid);
  ep.init(p, 0, zs);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn0 + j * 32 + fc;
    const bool nok = n < Nn;
    ep.col(p, nok ? n : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] *= unscale;
      ep.strip(p, m0 + wm0 + i * 32 + 4 * fk, M, nok, nok ? n : 0, acc[i][j]);
    }
  }
}

// The fp32 row loaders of the weight gradients (addressing only; RowsA / RowsBT add the split and the LDS store).
// Operands: rows = channels, k = pixels (contiguous in NCHW).  Thread (row = tid>>1, half = tid&1) holds the
// 16 consecutive pixels k0 + 16*half .. +15 of its channel, shifted by the tap for the x operand.  Requires W a
// power of two >= 4 and H*W a power of two >= 16; SEG = min(W, 16): a 16-pixel run is 16 / SEG whole row segments.
// With a concat input the first source must hold a multiple of 32 channels (a wave's 32 rows share one tensor).
template <bool SHIFT, bool DUAL, int SEG>
struct RowsLoader {
  static_assert(SEG == 16 || SEG == 8 || SEG == 4, "row segment of a 16-pixel run");
  static constexpr int NSEG = 16 / SEG;
  __amdgpu_buffer_rsrc_t rs;
  int rowoff;             // element offset of this thread's channel plane inside image 0 of its tensor
  int bstride;            // elements between images in this thread's tensor
  int row, half, dy, dx; bool rowok; unsigned okm;
  float r[16];
  __device__ __forceinline__ void init(const ConvP& p, const Src&, int o0, int tid, int zb) {
    row = tid >> 1; half = tid & 1; okm = 0;
    dy = SHIFT ? zb / 3 - 1 : 0; dx = SHIFT ? zb % 3 - 1 : 0;     // (a 1x1 layer passes the centre tap, zb = 4)
    const int ch = o0 + row;
    if (SHIFT) {                                   // x: channel of the concat input
      rowok = ch < p.Cin;
      const int c = rowok ? ch : 0;
      const bool first = !DUAL || __builtin_amdgcn_readfirstlane(o0 + (tid >> 6) * 32) < p.C1;   // wave-uniform
      rs = first ? make_rsrc(p.x1, (long)p.N * p.C1 * p.HW * 4) : make_rsrc(p.x2, (long)p.N * p.C2 * p.HW * 4);
      rowoff = (first ? c : (c >= p.C1 ? c - p.C1 : 0)) * p.HW;
      bstride = (first ? p.C1 : p.C2) * p.HW;
    } else {                                       // dy: output channel
      rowok = ch < p.Cout;
      rs = make_rsrc(p.dy, (long)p.N * p.Cout * p.HW * 4);
      rowoff = (rowok ? ch : 0) * p.HW;
      bstride = p.Cout * p.HW;
    }
  }
  // slice 14 computes the next run's mask and offsets, slices 15..19 issue its loads (all 16 registers were
  // consumed by the conversion slices 0..7); the mask in use by those slices is replaced at slice 14.
  unsigned os[NSEG], og[NSEG];      // byte offsets of the first element / of elements 1.. of each row segment
  __device__ __forceinline__ void ld(int g, const ConvP& p, const Src&, int c) {
    if (g == 14) {
      const int k = c * KC + half * 16;              // first pixel of the run (global pixel index)
      const bool kin = rowok && k < p.N * p.HW;      // N*H*W is a multiple of 16: a run is inside or outside as a whole
      const int b = k >> p.ohw_shift, hw = k & (p.HW - 1);
      const int y = hw >> p.ow_shift, x0 = hw & (p.W - 1);
      unsigned m = 0;
      if (!SHIFT) {
        m = 0xffffu;
      } else if (SEG == 16) {                        // one row segment of a row of >= 16 pixels
        const bool yok = (unsigned)(y + dy) < (unsigned)p.H;
        m = yok ? 0xffffu : 0u;
        if (dx < 0 && x0 == 0) m &= ~1u;
        if (dx > 0 && x0 + 16 == p.W) m &= ~0x8000u;
      } else {                                       // NSEG whole rows of SEG pixels
#pragma unroll
        for (int sgi = 0; sgi < NSEG; ++sgi)
          if ((unsigned)(y + sgi + dy) < (unsigned)p.H) m |= ((1u << SEG) - 1u) << (sgi * SEG);
        constexpr unsigned FIRST = SEG == 8 ? 0x0101u : 0x1111u;
        if (dx < 0) m &= ~FIRST;
        if (dx > 0) m &= ~(FIRST << (SEG - 1));
      }
      okm = kin ? m : 0u;
      // The run is contiguous in memory, but its element offsets may be negative where they are masked: column -1
      // of the first row of the tensor (the first element of a segment), or whole leading segments when the row
      // above the image is addressed.  A negative voffset plus an immediate is NOT wrapped back into the buffer by
      // the range check, so each segment is read as two pieces -- its first element and the rest -- each from its
      // own offset clamped at 0 (a clamped piece is entirely masked), immediates only inside a piece.  The offsets
      // are made opaque because hipcc otherwise rewrites max(o + 1, 0) * 4 + imm as max(o, -1) * 4 + (imm + 4),
      // i.e. back into the negative-base form.  A run that ends past the tensor reads 0 there (range check).
      const int o = (kin ? b * bstride + rowoff + hw : 0) + dy * p.W + dx;
#pragma unroll
      for (int sgi = 0; sgi < NSEG; ++sgi) {
        os[sgi] = (unsigned)(max(o + sgi * SEG, 0) * 4);
        og[sgi] = (unsigned)(max(o + sgi * SEG + 1, 0) * 4);
        asm volatile("" : "+v"(os[sgi]), "+v"(og[sgi]));
      }
    } else if (g == 15) {
#pragma unroll
      for (int sgi = 0; sgi < NSEG; ++sgi) r[sgi * SEG] = bload(rs, os[sgi], 0);
    } else if (g >= 16 && g < 20) {
      // the 16 - NSEG remaining elements in four slices: quarter q of every segment's tail
      const int q = g - 16;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int sgi = j / SEG, e = j % SEG;                     // element e >= 1 of segment sgi
        if (e >= 1 && ((e - 1) * 4) / (SEG - 1) == q) r[j] = bload(rs, og[sgi] + (unsigned)(e - 1) * 4u, 0);
      }
    }
  }
};

// ---- 3x3 weight gradient, three taps per workgroup -------------------------------------------------------------------
// A workgroup owns one kernel ROW (kh) of a 128(co) x 64(ci) block of dw: the three taps kw = 0, 1, 2 read the same x pixels
// shifted by one, so a thread loads its 8-pixel run plus one pixel on each side ONCE, splits those 10 values once and writes
// the three shifted windows to LDS; the dy tile is staged once for all three taps.  Both operands are scaled and split into
// two fp16 terms: 18 MFMAs per wave and half chunk.
//   A tile  [2 planes][128 co][32 px]            RowsA (unshifted dy rows)
//   B tiles [3 taps][2 planes][64 ci][32 px]     Rows3: thread (row = tid >> 2, quarter = tid & 3) owns pixels 8q .. 8q + 7
// Waves: 2 (co halves of 64 rows = 2 MFMA tiles) x 2 (ci halves of 32 = 1 MFMA tile); accumulators acc[2][3 taps].
// Requires W a power of two >= 8 (an 8-pixel run stays inside one image row), H*W a power of two >= 32.
constexpr int W3_BPLANE = 64 * PITCH;
constexpr int W3_BTAP = 2 * W3_BPLANE;
constexpr int W3_LDS = OPER + 3 * W3_BTAP;       // 20480 + 30720 = 51200 bytes

// Rows3's addressing: the x run of 8 pixels plus the one on each side, for the three taps of kernel row kh
template <bool DUAL>
struct Rows3Loader {
  float r[10];             // elements -1 .. 8  (first: the member layout steers wgrad3_kernel's schedule)
  __amdgpu_buffer_rsrc_t rs;
  int rowoff, bstride, row, quarter, dy; bool rowok;
  unsigned okm;            // bit e + 1: element e (-1 .. 8) of the current run is valid
  unsigned om, o0, o8;
  __device__ __forceinline__ void init(const ConvP& p, int n0, int tid, int kh) {
    row = tid >> 2; quarter = tid & 3; dy = kh - 1; okm = 0;
    const int ch = n0 + row;
    rowok = ch < p.Cin;
    const int c = rowok ? ch : 0;
    const bool first = !DUAL || __builtin_amdgcn_readfirstlane(n0 + (tid >> 6) * 16) < p.C1;   // wave-uniform
    rs = first ? make_rsrc(p.x1, (long)p.N * p.C1 * p.HW * 4) : make_rsrc(p.x2, (long)p.N * p.C2 * p.HW * 4);
    rowoff = (first ? c : (c >= p.C1 ? c - p.C1 : 0)) * p.HW;
    bstride = (first ? p.C1 : p.C2) * p.HW;
  }
  // slice 14: mask and offsets of the next run; 15: the two halo elements; 16, 17: the eight pixels of the run
  __device__ __forceinline__ void ld(int g, const ConvP& p, int c) {
    if (g == 14) {
      const int k = c * KC + quarter * 8;
      const bool kin = rowok && k < p.N * p.HW;
      const int b = k >> p.ohw_shift, hw = k & (p.HW - 1);
      const int y = hw >> p.ow_shift, x0 = hw & (p.W - 1);
      unsigned m = (unsigned)(y + dy) < (unsigned)p.H ? 0x3ffu : 0u;
      if (x0 == 0) m &= ~1u;                       // column -1
      if (x0 + 8 == p.W) m &= ~0x200u;             // column W
      okm = kin ? m : 0u;
      // offsets clamped at 0 and opaque, pieces [-1], [0..7], [8]: see RowsLoader
      const int o = (kin ? b * bstride + rowoff + hw : 0) + dy * p.W;
      om = (unsigned)(max(o - 1, 0) * 4); o0 = (unsigned)(max(o, 0) * 4); o8 = (unsigned)(max(o + 8, 0) * 4);
      asm volatile("" : "+v"(om), "+v"(o0), "+v"(o8));
    } else if (g == 15) {
      r[0] = bload(rs, om, 0);
      r[9] = bload(rs, o8, 0);
    } else if (g == 16 || g == 17) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[1 + (g - 16) * 4 + j] = bload(rs, o0 + (unsigned)((g - 16) * 4 + j) * 4u, 0);
    }
  }
};

struct RowsA : RowsLoader<false, false, 16> {          // dy: 16 consecutive pixels of one output channel
  Split16 sp2; float scale;
  __device__ __forceinline__ void st(int g, unsigned char* t) { sp2.st(g, r, scale, t, row, half * 16, okm); }
};

template <bool DUAL>
struct Rows3 : Rows3Loader<DUAL> {                     // x: the 10-pixel run of one input channel, three windows
  using B = Rows3Loader<DUAL>;
  _Float16 hh[2][10]; float scale;
  // slices 0..4 split two elements each, 5..10 pack + write one (tap, plane) window each
  __device__ __forceinline__ void st(int g, unsigned char* t) {
    if (g < 5) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = 2 * g + u;
        const float v = scale * igemm::keep_if(B::r[e], B::okm, e);
        hh[0][e] = (_Float16)v;
        hh[1][e] = (_Float16)(v - (float)hh[0][e]);
      }
    } else if (g < 11) {
      const int tap = (g - 5) >> 1, s = (g - 5) & 1;        // window of tap kw: elements kw - 1 .. kw + 6 -> hh[kw .. kw + 7]
      unsigned char* d = t + tap * W3_BTAP + s * W3_BPLANE + B::row * PITCH + B::quarter * 16;
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const halfx2 v = {hh[s][tap + 2 * j], hh[s][tap + 2 * j + 1]};
        w[j] = __builtin_bit_cast(unsigned, v);
      }
      *reinterpret_cast<u32x4*>(d) = u32x4{w[0], w[1], w[2], w[3]};
    }
  }
};

// dypart: 256 partial |dy| maxima; xpart: nxpart (256 / 512) partial |x| maxima
template <bool DUAL>
__global__ __launch_bounds__(256) void wgrad3_kernel(ConvP p, int tiles_m, int tiles_n, int nchunks_total, int chunks_per_split,
                                                     const float* __restrict__ dypart, const float* __restrict__ xpart, int nxpart) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[W3_LDS];
  unsigned char* As = lds;
  unsigned char* Bs = lds + OPER;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const float sa = pow2_scale_of(block_amax(dypart, NPART, reinterpret_cast<float*>(lds)));
  const float sb = pow2_scale_of(block_amax(xpart, nxpart, reinterpret_cast<float*>(lds)));
  const float unscale = (1.f / sa) / sb;      // in turn: sa sb may pass 2^127
  const int ntiles = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, gridDim.x);       // kernel row fastest: the three blocks share dy / x panels
  const int kh = id % 3;
  const int rest = id / 3;
  const int tile = rest % ntiles;
  const int zs = rest / ntiles;
  const int tm = tile % tiles_m, tn = tile / tiles_m;
  const int m0 = tm * 128, n0 = tn * 64;
  const int c_begin = zs * chunks_per_split;
  const int c_last = min(nchunks_total, c_begin + chunks_per_split) - 1;

  Src q = {};
  RowsA al;
  Rows3<DUAL> bl;
  al.init(p, q, m0, tid, 4); al.scale = sa;
  bl.init(p, n0, tid, kh); bl.scale = sb;

  floatx16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][t][e] = 0.f;

  const int wm0 = (wid & 1) * 64, wn0 = (wid >> 1) * 32;
  const int fk = lane >> 5, fc = lane & 31;
  const unsigned char* a_rd = As + (wm0 + fc) * PITCH + fk * 16;
  const unsigned char* b_rd = Bs + (wn0 + fc) * PITCH + fk * 16;

#define STK_W3_FRAGS(KK)                                                                                   \
  _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                           \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                            \
      a[i][s] = *reinterpret_cast<const halfx8*>(a_rd + s * PLANE + i * 32 * PITCH + (KK) * 32);             \
    _Pragma("unroll") for (int t = 0; t < 3; ++t)                                                            \
      b[t][s] = *reinterpret_cast<const halfx8*>(b_rd + t * W3_BTAP + s * W3_BPLANE + (KK) * 32);            \
  }
  constexpr int SA[3] = {1, 0, 0}, SB[3] = {0, 1, 0};
#define STK_W3_MFMAS                                                                                       \
  _Pragma("unroll") for (int pr = 0; pr < 3; ++pr) _Pragma("unroll") for (int i = 0; i < 2; ++i)              \
    _Pragma("unroll") for (int t = 0; t < 3; ++t)                                                            \
      acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][SA[pr]], b[t][SB[pr]], acc[i][t], 0, 0, 0);

#pragma unroll
  for (int g = 0; g < 24; ++g) { al.ld(g, p, q, c_begin); bl.ld(g, p, c_begin); }
  {
    const int c1 = min(c_begin + 1, c_last);
#pragma unroll
    for (int g = 0; g < 24; ++g) { al.st(g, As); bl.st(g, Bs); }
#pragma unroll
    for (int g = 0; g < 24; ++g) { al.ld(g, p, q, c1); bl.ld(g, p, c1); }
  }
  halfx8 a[2][2], b[3][2];
  for (int c = c_begin; c < c_last; ++c) {
    __syncthreads();                                   // chunk c is in LDS
    STK_W3_FRAGS(0)
    STK_W3_MFMAS
    STK_W3_FRAGS(1)
    __syncthreads();                                   // nobody reads LDS any more
    const int c2 = min(c + 2, c_last);
    STK_W3_MFMAS
#pragma unroll
    for (int g = 0; g < 24; ++g) al.st(g, As);
#pragma unroll
    for (int g = 0; g < 24; ++g) bl.st(g, Bs);
#pragma unroll
    for (int g = 0; g < 24; ++g) al.ld(g, p, q, c2);
#pragma unroll
    for (int g = 0; g < 24; ++g) bl.ld(g, p, c2);
#pragma unroll
    for (int g = 0; g < 18; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 9, 0);     // VALU
      if (g < 10) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write (4 + 6 per thread and chunk)
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);     // VMEM read
    }
  }
  __syncthreads();
  STK_W3_FRAGS(0)
  STK_W3_MFMAS
  STK_W3_FRAGS(1)
  STK_W3_MFMAS
#undef STK_W3_MFMAS
#undef STK_W3_FRAGS

  // partial slab of split zs as [tap][Cout][Cin] (lanes = ci, contiguous); splitk_reduce_kernel re-lays it out
  float* slab = p.part + (long)zs * p.part_stride;
  const int n = n0 + wn0 + fc;
  if (n < p.Cin) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wm0 + i * 32 + 4 * fk + igemm::strip_row(e);
          if (m < p.Cout) slab[((long)(kh * 3 + t) * p.Cout + m) * p.Cin + n] = unscale * acc[i][t][e];
        }
  }
}

// ---- per-tap weight gradient (1x1 layers, 3x3 on 4-wide maps) ------------------------------------------------------------
// One 128 x 128 tile of one tap per workgroup, rows = output channels (dy), columns = input channels (x), k = pixels; both
// operands scaled and split into two fp16 terms: 12 MFMAs per 16-k step.  With so few MFMAs the conversions do not hide
// behind one half-chunk alone, so a chunk's work is laid out over both halves: the split of chunk
// c + 1 (registers only) and the load issue of chunk c + 2 ride on the MFMAs of kk = 0, the eight LDS stores on those of
// kk = 1 (after the barrier that retires the reads of chunk c).
template <bool DUAL, int SEG, bool X1>
struct RowsBT : RowsLoader<true, DUAL, SEG> {          // x: 16 consecutive (tap-shifted) pixels of one input channel
  using B = RowsLoader<true, DUAL, SEG>;
  Split16X<X1> sp2; float scale;
  __device__ __forceinline__ void st(int g, unsigned char* t) { sp2.st(g, B::r, scale, t, B::row, B::half * 16, B::okm); }
};
template <bool DUAL, int SEG> struct RowsB : RowsBT<DUAL, SEG, false> {};
template <bool DUAL, int SEG> struct RowsB16 : RowsBT<DUAL, SEG, true> {};     // hi plane only (OneProduct weight gradient)

// Unshifted rows (dy always; x of a 1x1 layer): the thread's 16 consecutive pixels are one aligned 64-byte run, read as
// four 16-byte loads.  (RowsLoader reads a run element by element because a tap shift breaks the alignment and needs
// a per-element mask; with 32 such loads per thread and chunk, each touching 64 separate 64-byte segments, the per-tap
// kernel was bound by address processing: 54 us for the 256 -> 256 layer at 16 x 16 against ~6 us of MFMAs.)
template <bool IS_X, bool DUAL, bool X1>
struct RowsUT {
  __amdgpu_buffer_rsrc_t rs;
  int rowoff, bstride, row, half; bool rowok; unsigned voff;
  float r[16]; Split16X<X1> sp2; float scale;
  __device__ __forceinline__ void init(const ConvP& p, const Src&, int o0, int tid, int) {
    row = tid >> 1; half = tid & 1; voff = 0x80000000u;
    const int ch = o0 + row;
    if (IS_X) {
      rowok = ch < p.Cin;
      const int c = rowok ? ch : 0;
      const bool first = !DUAL || __builtin_amdgcn_readfirstlane(o0 + (tid >> 6) * 32) < p.C1;   // wave-uniform
      rs = first ? make_rsrc(p.x1, (long)p.N * p.C1 * p.HW * 4) : make_rsrc(p.x2, (long)p.N * p.C2 * p.HW * 4);
      rowoff = (first ? c : (c >= p.C1 ? c - p.C1 : 0)) * p.HW;
      bstride = (first ? p.C1 : p.C2) * p.HW;
    } else {
      rowok = ch < p.Cout;
      rs = make_rsrc(p.dy, (long)p.N * p.Cout * p.HW * 4);
      rowoff = (rowok ? ch : 0) * p.HW;
      bstride = p.Cout * p.HW;
    }
  }
  // slice 14: the run's byte offset (bit 31 = outside: the loads return 0); slices 15..18: one 16-byte load each
  __device__ __forceinline__ void ld(int g, const ConvP& p, const Src&, int c) {
    if (g == 14) {
      const int k = c * KC + half * 16;
      const bool kin = rowok && k < p.N * p.HW;
      const int b = k >> p.ohw_shift, hw = k & (p.HW - 1);
      voff = kin ? (unsigned)((b * bstride + rowoff + hw) * 4) : 0x80000000u;
    } else if (g >= 15 && g < 19) {
      const int j = g - 15;
      const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, j * 16, 0));
      r[4 * j] = __uint_as_float(v[0]); r[4 * j + 1] = __uint_as_float(v[1]);
      r[4 * j + 2] = __uint_as_float(v[2]); r[4 * j + 3] = __uint_as_float(v[3]);
    }
  }
  __device__ __forceinline__ void st(int g, unsigned char* t) { sp2.st(g, r, scale, t, row, half * 16); }
};
template <bool IS_X, bool DUAL> struct RowsU : RowsUT<IS_X, DUAL, false> {};
template <bool IS_X, bool DUAL> struct RowsU16 : RowsUT<IS_X, DUAL, true> {};  // hi plane only (OneProduct weight gradient)

// X1 (EP = OneProduct<EpWgrad>, include/stk_fp16_train.h): RowsU16 / RowsB16 loaders, split-0 fragments only, and the 4
// hi(dy) hi(x) MFMAs of the 12 per half chunk.
template <class AL, class BL, class EP, bool PIN>
__global__ __launch_bounds__(256) void wgemm_kernel(ConvP p, int M, int Nn, int tiles_m, int tiles_n, int nchunks_total,
                                                    int chunks_per_split, int taps_z, const float* __restrict__ dypart,
                                                    const float* __restrict__ xpart, int nxpart) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  constexpr bool X1 = is_x1<EP>::value;
  unsigned char* As = lds;
  unsigned char* Bs = lds + OPER;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const float sa = pow2_scale_of(block_amax(dypart, NPART, reinterpret_cast<float*>(lds)));
  const float sb = pow2_scale_of(block_amax(xpart, nxpart, reinterpret_cast<float*>(lds)));
  const float unscale = (1.f / sa) / sb;      // in turn: sa sb may pass 2^127
  const int ntiles = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int zb = id % taps_z;
  const int rest = id / taps_z;
  const int tile = rest % ntiles;
  const int zs = rest / ntiles;
  const int tm = tile % tiles_m, tn = tile / tiles_m;
  const int m0 = tm * 128, n0 = tn * 128;
  const int c_begin = zs * chunks_per_split;
  const int c_last = min(nchunks_total, c_begin + chunks_per_split) - 1;

  Src q = {};
  AL al; BL bl;
  al.init(p, q, m0, tid, 4); al.scale = sa;
  bl.init(p, q, n0, tid, taps_z == 1 ? 4 : zb); bl.scale = sb;

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int wm0 = (wid & 1) * 64, wn0 = (wid >> 1) * 64;
  const int fk = lane >> 5, fc = lane & 31;
  const unsigned char* a_rd = As + (wm0 + fc) * PITCH + fk * 16;
  const unsigned char* b_rd = Bs + (wn0 + fc) * PITCH + fk * 16;

#define STK_W1_FRAGS(KK)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int s = 0; s < (X1 ? 1 : 2); ++s) {         \
    a[i][s] = *reinterpret_cast<const halfx8*>(a_rd + s * PLANE + i * 32 * PITCH + (KK) * 32);          \
    b[i][s] = *reinterpret_cast<const halfx8*>(b_rd + s * PLANE + i * 32 * PITCH + (KK) * 32);          \
  }
  constexpr int SA[3] = {1, 0, 0}, SB[3] = {0, 1, 0};
#define STK_W1_MFMA(G)                                                                                              \
  if (!X1 || ((G) >> 2) == 2)                                                                                       \
  acc[((G) >> 1) & 1][(G) & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[((G) >> 1) & 1][SA[(G) >> 2]], b[(G) & 1][SB[(G) >> 2]], \
                                                                        acc[((G) >> 1) & 1][(G) & 1], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 24; ++g) { al.ld(g, p, q, c_begin); bl.ld(g, p, q, c_begin); }
#pragma unroll
  for (int g = 0; g < 12; ++g) { al.st(g, As); bl.st(g, Bs); }
  {
    const int c1 = min(c_begin + 1, c_last);
#pragma unroll
    for (int g = 0; g < 24; ++g) { al.ld(g, p, q, c1); bl.ld(g, p, q, c1); }
  }
  halfx8 a[2][2], b[2][2];
  for (int c = c_begin; c < c_last; ++c) {
    __syncthreads();                                   // chunk c is in LDS
    STK_W1_FRAGS(0)
#pragma unroll
    for (int g = 0; g < 12; ++g) { STK_W1_MFMA(g) }
#pragma unroll
    for (int g = 0; g < 8; ++g) { al.st(g, As); bl.st(g, Bs); }            // split of chunk c + 1: registers only
    const int c2 = min(c + 2, c_last);
#pragma unroll
    for (int g = 0; g < 24; ++g) { al.ld(g, p, q, c2); bl.ld(g, p, q, c2); }   // chunk c + 2: global -> registers
    if (PIN) {
#pragma unroll
      for (int g = 0; g < 12; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 18, 0);    // VALU
        __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);     // VMEM read
      }
    }
    STK_W1_FRAGS(1)
    __syncthreads();                                   // nobody reads chunk c any more
#pragma unroll
    for (int g = 0; g < 12; ++g) { STK_W1_MFMA(g) }
#pragma unroll
    for (int g = 8; g < 12; ++g) { al.st(g, As); bl.st(g, Bs); }           // chunk c + 1 -> LDS
    if (PIN) {
#pragma unroll
      for (int g = 0; g < 12; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (g >= 2 && g < 10) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
      }
    }
  }
  __syncthreads();
  STK_W1_FRAGS(0)
#pragma unroll
  for (int g = 0; g < 12; ++g) { STK_W1_MFMA(g) }
  STK_W1_FRAGS(1)
#pragma unroll
  for (int g = 0; g < 12; ++g) { STK_W1_MFMA(g) }
#undef STK_W1_MFMA
#undef STK_W1_FRAGS

  EP ep;
  ep.init(p, zb, zs);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn0 + j * 32 + fc;
    const bool nok = n < Nn;
    ep.col(p, nok ? n : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] *= unscale;
      ep.strip(p, m0 + wm0 + i * 32 + 4 * fk, M, nok, nok ? n : 0, acc[i][j]);
    }
  }
}

}  // namespace x2
