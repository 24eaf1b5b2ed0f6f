// stream.h -- what the HBM-bound streaming kernels share (elementwise.hip, impute.hip, solver.hip, superres.hip, cond.hip and,
// through rowsum.h, the per-sample files adaptive.hip, posterior.hip, guided.hip, edm.hip, consistency.hip, flow.hip).
//
// The layout they all follow: lanes walk consecutive addresses, 16 B per lane (one float4) whenever the length -- or the
// plane or row a thread stays inside -- is a multiple of 4 and every pointer given is 16-byte aligned, a scalar path
// otherwise; blocks of 256 threads, the grid capped by stk_ew_grid (common.h) and striding the rest.  A kernel is a
// template over V = 4 or 1 elements per item and moves its data through Vec<V>; its entry decides `vec` from its own length
// condition and stk_all_aligned16 of its pointers, and launches the pair through stk_launch_vec.
//
// Loads, stores and host code only: NO floating-point arithmetic belongs in this file.  The files that include it switch
// contraction off with a pragma that holds "for every function that follows" it, so arithmetic written here, before that
// pragma, would be compiled under another rule than the file that includes it states.  Headers that hold arithmetic
// (rowsum.h, sqloss.h) are included after the pragma.
#pragma once
#include "common.h"

// V consecutive floats of item i (elements [V i, V i + V)); the index type is the caller's (long in elementwise.hip,
// unsigned where the entry has checked that everything fits 32 bits).
template <int V> struct Vec;
template <> struct Vec<1> {
  float v[1];
  template <class I> __device__ static Vec load(const float* p, I i) { Vec r; r.v[0] = p[i]; return r; }
  template <class I> __device__ void store(float* p, I i) const { p[i] = v[0]; }
};
template <> struct Vec<4> {
  float v[4];
  template <class I> __device__ static Vec load(const float* p, I i) {
    float4 t = reinterpret_cast<const float4*>(p)[i];
    Vec r; r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; return r;
  }
  template <class I> __device__ void store(float* p, I i) const {
    reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// Every pointer given is 16-byte aligned.  An optional operand that is absent (null) counts as aligned.
template <class... P>
static inline bool stk_all_aligned16(const P*... p) { return (stk_aligned16(p) && ...); }

// Launch the 16-byte (k4) or the scalar (k1) instantiation of one kernel with 256 threads per block -> STK_OK / STK_ELAUNCH.
template <class K, class... A>
static inline int stk_launch_vec(bool vec, K k4, K k1, dim3 grid, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(vec ? k4 : k1, grid, dim3(256), 0, stream, args...);
  STK_CHECK_LAUNCH();
  return STK_OK;
}
