/*
 * stk_adaptive.h -- the three passes of the adaptive-step SDE sampler of libstk (Jolicoeur-Martineau et al., "Gotta Go Fast
 * When Generating Data with Score-Based Models", 2021): an Euler-Maruyama stage, the stochastic improved-Euler step with its
 * per-sample mixed-tolerance error, and the per-sample accept / reject with the step-size controller.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a sampler that needs them on
 * a library without them is refused when it is built, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * The state is B samples, rows of n = C H W contiguous floats.  Every sample b has its own time t_b and step h_b, fp32
 * vectors in DEVICE memory, and so are the coefficient rows: nothing per-sample travels through the host.  With the forward
 * SDE dx = c(t) x dt + g(t) dw and t' = t - h, one iteration is
 *
 *   x1  = (1 - h c(t)) x + h g(t)^2 s1 + sqrt(h) g(t) z                 stk_sde_stage_f32, row (1 - h c, 0, h g^2, sqrt(h) g)
 *   xt  = x - h c(t') x1 + h g(t')^2 s2 + sqrt(h) g(t') z               stk_sde_heun_error_f32, row (1, -h c', h g'^2, sqrt(h) g')
 *   x2  = (x1 + xt) / 2
 *   d   = max(atol, rtol max(|x1|, |x1_prev|))
 *   E_b = sqrt(mean over the row of ((x1 - x2) / d)^2)
 *   accept / reject, t_b, h_b, x <- x2 and x1_prev <- x1 where accepted  stk_sde_commit_f32
 *
 * Arithmetic.  Every element-wise expression is evaluated in fp32 in the order written, left to right, each product and
 * each sum rounded once: no fused multiply-add, so a restatement in plain fp32 arithmetic reproduces x1, x2 and every
 * ((x1 - x2) / d)^2 bit for bit.  The squares are summed in float64 (the error norm of one sample has up to 2^31
 * terms), per thread, per block and across blocks in a fixed order: no floating-point atomics, E_b is bit-identical from
 * run to run.  The power of the controller is evaluated in float64 and rounded once.
 *
 * 16-byte accesses are used when n is a multiple of 4 and every pointer given is 16-byte aligned (then every row starts
 * aligned); a scalar path otherwise.  That is decided per launch.
 */
#ifndef STK_ADAPTIVE_H
#define STK_ADAPTIVE_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of stk_sde_heun_error_f32 / stk_sde_commit_f32 for B rows of n_per_sample floats: the float64
 * partial sums, one per (sample, block); a function of the two sizes alone, not of the alignment.  Negative where the other
 * entries refuse: STK_EINVAL for B <= 0 or n_per_sample <= 0, STK_EUNSUPPORTED for B n_per_sample >= 2^31. */
long stk_sde_ws_bytes(int B, long n_per_sample);

/* out[b, :] = (coef[b,0] x[b, :] + coef[b,1] xp[b, :]) + coef[b,2] score[b, :] + coef[b,3] z[b, :], summed in that order.
 * coef: [B, 4] floats on the device.  xp may be NULL: its term is then left out (coef[b,1] is not read).  out overlaps no
 * operand.
 * STK_EINVAL: x, score, z, coef or out NULL, B <= 0, n <= 0.  STK_EUNSUPPORTED: B n >= 2^31. */
int stk_sde_stage_f32(const float* x, const float* xp, const float* score, const float* z, const float* coef, float* out,
                      int B, long n, void* stream);

/* xt = ((coef[b,0] x + coef[b,1] x1) + coef[b,2] score2) + coef[b,3] z;  x2 = 0.5 (x1 + xt);
 * d = max(atol, rtol max(|x1|, |x1_prev|));  q = (x1 - x2) / d;  the workspace receives, per sample and block, the float64
 * sum of the block's fp32 q q.  Writes x2 [B, n] and the workspace (every slot, every launch: nothing has to be zeroed);
 * x2 overlaps no operand.  ws: at least stk_sde_ws_bytes(B, n) bytes, 8-byte aligned.
 * STK_EINVAL: a NULL pointer, B <= 0, n <= 0, atol or rtol negative or NaN or both zero, ws_bytes too small, ws
 * misaligned.  STK_EUNSUPPORTED: B n >= 2^31. */
int stk_sde_heun_error_f32(const float* x, const float* x1, const float* x1_prev, const float* score2, const float* z,
                           const float* coef, float atol, float rtol, float* x2, void* ws, long ws_bytes, int B, long n,
                           void* stream);

/* Per sample b, from the workspace stk_sde_heun_error_f32 left (same B and n):
 *   E        = sqrt(sum of the partials, in index order within a fixed tree / n)
 *   active   = t > eps                             a sample at eps is finished: it stays as it is, with h_out = 0
 *   accept   = active and E <= 1                   a NaN or infinite E is a rejection
 *   t'       = eps if h >= t - eps, else t - h     a clamped step lands on eps exactly, never below it
 *   t_out    = t' if accept, else t
 *   h_out    = min(t_out - eps, safety h E^-exponent)     active, E finite (E = 0: the first operand)
 *            = min(t_out - eps, safety h / 2)             active, E not finite
 *            = 0                                          finished
 *   x[b, :] <- x2[b, :] and x1_prev[b, :] <- x1[b, :]     accepted samples only; every other row is not written
 * E_out [B] floats and accept_out [B] ints (1 / 0) stay on the device.  t_out and h_out are vectors of their own: they must
 * not be t or h (no block reads what another writes).  x and x1_prev overlap neither x2 nor x1.
 * STK_EINVAL: a NULL pointer, B <= 0, n <= 0, t_out or h_out equal to t or h, eps negative or NaN, safety not positive,
 * exponent negative or NaN, ws_bytes too small, ws misaligned.  STK_EUNSUPPORTED: B n >= 2^31. */
int stk_sde_commit_f32(float* x, float* x1_prev, const float* x2, const float* x1, const float* t, const float* h,
                       float eps, float safety, float exponent, const void* ws, long ws_bytes, float* t_out, float* h_out,
                       float* E_out, int* accept_out, int B, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
