/*
 * stk_flow.h -- the element-wise work of rectified flow in libstk (Liu, Gong and Liu, "Flow Straight and Fast: Learning to
 * Generate and Transfer Data with Rectified Flow", 2022; Lipman et al., "Flow Matching for Generative Modeling", 2022): the
 * velocity loss with its gradient, and the one launch that serves the Euler, Heun and stochastic steps of the sampler.  The
 * network v runs between these launches; it is the caller's.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a loss that needs them on a
 * library without them takes its torch-expression path, a sampler is refused when it is built.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * The interpolant between data y (t = 0) and noise n (t = 1) is the straight line x_t = (1 - t) y + t n; the network predicts
 * its velocity dx_t/dt = n - y.  A training evaluation on B samples of `inner` = C H W floats, with times t[B]:
 *
 *   x_t            = a y + t n,  a = 1 - t                          stk_perturb_f32 of stk.h
 *   F              = network(x_t, t)                                the caller's
 *   r              = F - (n - y),  loss[b] = sum r^2  (/ inner)     stk_flow_loss_f32
 *   dF             = (2 dloss_b (/ inner)) r                        stk_flow_loss_grad_f32
 *
 * The sampler integrates dx/dt = v(x, t) from t_0 = 1 down to t_steps = 0.  Where the step's row comes from: in tau = 1 - t
 * the marginals p_t of the interpolant are kept by every member of the family
 *
 *   dx = [-v + (w / 2) score] dtau + sqrt(w) dW,   w >= 0,
 *
 * since the Fokker-Planck equation of this SDE differs from that of dx = -v dtau by div(p (w / 2) score) - (w / 2) lap p = 0.
 * For the Gaussian bridge score(x, t) = -(x + (1 - t) v) / t, singular at t = 0; with w = 2 eta t the 1 / t cancels:
 *
 *   dx = [-v - eta (x + (1 - t) v)] dtau + sqrt(2 eta t) dW.
 *
 * One Euler-Maruyama step of length D = t_i - t_{i+1} is x' = cx x + cv v + cn eps with
 *
 *   cx = 1 - eta D,   cv = -D (1 + eta (1 - t_i)),   cn = sqrt(2 eta t_i D);
 *
 * eta = 0 is the ODE's Euler step (1, -D, 0).  Heun's correction reuses that row on the mean of the two velocities.  All
 * three are one launch:
 *
 *   x' = x + cv v                                                   stk_flow_step_f32, Euler: reads x, v; writes x'     12 B
 *   x  = x + cv (v / 2 + v' / 2)                                    ..., the correction: v_prev = v, in place          16 B
 *   x  = cx x + cv v + cn eps                                       ..., the stochastic step, in place                  16 B
 *
 * v_prev is the network's own output of the Euler stage: no slope is ever written.  cx = 1 is an exact product, so the
 * deterministic forms are x + cv slope bit for bit.
 *
 * Arithmetic.  Every element-wise expression is evaluated in fp32 in the order written at its entry below, each product and
 * sum rounded once: no fused multiply-add, so a restatement in plain fp32 arithmetic reproduces every element bit for bit.
 * The squares r r are summed in float64, per thread, per block and across blocks in a fixed order: no floating-point
 * atomics, loss_out is bit-identical from run to run.
 *
 * 16-byte accesses are used when the row length (inner; n for the sampler's entry) is a multiple of 4 and every pointer
 * given is 16-byte aligned; a scalar path otherwise.  That is decided per launch.
 */
#ifndef STK_FLOW_H
#define STK_FLOW_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of stk_flow_loss_f32 for B rows of inner floats: the float64 partial sums, one per (sample, block);
 * a function of the two sizes alone, not of the alignment.  Negative where the other entries refuse: STK_EINVAL for B <= 0 or
 * inner <= 0, STK_EUNSUPPORTED for B inner >= 2^31. */
long stk_flow_ws_bytes(int B, long inner);

/* On [B, inner]:
 *   u = n - y;  r = F - u;  q = r r
 * The workspace receives, per sample and block, the float64 sum of the block's fp32 q (every slot, every launch: nothing has
 * to be zeroed); a finishing pass enqueued by the same call adds a row's partials in index order within a fixed tree to S and
 * writes loss_out[b] = (float)S, or (float)(S / (double)inner) under reduce_mean.
 * r_out receives r; it may be NULL (an evaluation without gradient), and overlaps no operand otherwise.
 * ws: at least stk_flow_ws_bytes(B, inner) bytes, 8-byte aligned.
 * STK_EINVAL: a NULL pointer other than r_out, B <= 0, inner <= 0, ws_bytes too small, ws misaligned.
 * STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_flow_loss_f32(const float* F, const float* y, const float* n, void* ws, long ws_bytes, float* r_out, float* loss_out,
                      int B, long inner, int reduce_mean, void* stream);

/* dF = k r on [B, inner] with k = 2 dloss[b] in fp32 (exact), and k = k / (float)inner after that under reduce_mean.  dF may
 * be r itself.
 * STK_EINVAL: a NULL pointer, B <= 0, inner <= 0.  STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_flow_loss_grad_f32(const float* r, const float* dloss, float* dF, int B, long inner, int reduce_mean, void* stream);

/* Every form of a sampler step, on n elements:
 *   slope = v_prev ? 0.5 v_prev + 0.5 v : v;  m = cx xb;  p = cv slope;  x = m + p;
 *   with eps:  x = x + cn eps;
 *   x_out = x
 * v_prev and eps may be NULL, and are not given together.  x_out may be xb: an item reads everything before it writes, and no
 * two items share an element.  No other overlap.
 * STK_EINVAL: xb, v or x_out NULL, n <= 0, eps NULL with cn != 0, cn negative or NaN, v_prev and eps both given.
 * STK_EUNSUPPORTED: n >= 2^31. */
int stk_flow_step_f32(const float* xb, const float* v, const float* v_prev, const float* eps, float cx, float cv, float cn,
                      float* x_out, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
