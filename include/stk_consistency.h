/*
 * stk_consistency.h -- the element-wise work of consistency training and consistency sampling in libstk (Song et al.,
 * "Consistency Models", 2023; Song & Dhariwal, "Improved Techniques for Training Consistency Models", 2023): the per-sample
 * coefficients of the consistency function at a pair of neighbouring noise levels, both network inputs of the pair from one
 * read of the data and the noise, the pseudo-Huber loss between the two evaluations with its gradient, and the one launch of
 * a sampler step.  The network F runs between these launches; it is the caller's.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a loss that needs them on a
 * library without them takes its torch-expression path, a sampler is refused when it is built.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * With s = sigma_data and e = sigma_min the consistency function at the noise level sigma is
 * f(x; sigma) = c_skip x + c_out F(c_in x; c_noise),
 *
 *   c_in = 1 / sqrt(sigma^2 + s^2),  c_skip = s^2 / ((sigma - e)^2 + s^2),  c_out = s (sigma - e) / sqrt(sigma^2 + s^2),
 *   c_noise = ln(sigma) / 4:  c_skip = 1 and c_out = 0 at sigma = e, so f(x; e) = x.
 *
 * A training evaluation on B samples y of `inner` = C H W floats, with ONE noise n and the level pairs sigma_hi > sigma_lo:
 *
 *   coef           = the eleven rows below                          stk_ct_coeffs_f32
 *   xin_hi, xin_lo = c_in y + (c_in sigma) n  at each level          stk_ct_pair_f32
 *   F_lo, F_hi     = network(xin, c_noise)  at each level            the caller's (F_lo without gradient)
 *   r              = f(y + sigma_hi n; sigma_hi) - f(y + sigma_lo n; sigma_lo),  S = sum r^2,
 *   loss[b]        = lambda S / (sqrt(S + c^2) + c)  (/ inner)       stk_ct_loss_f32
 *   dF_hi          = (gfac_b dloss_b) r                              stk_ct_loss_grad_f32
 *
 * with lambda = 1 / (sigma_hi - sigma_lo) and gfac = lambda c_out_hi / sqrt(S + c^2) (/ inner).  One step of the sampler at
 * the level tau, towards the next level tau' (none after the last):
 *
 *   F    = network(xin, c_noise(tau))                                the caller's
 *   x0   = clamp(c_skip(tau) x + c_out(tau) F, lo, hi)
 *   x    = x0 + sqrt(tau'^2 - e^2) z,  xin = c_in(tau') x             stk_ct_step_f32
 *
 * Arithmetic.  Every element-wise expression is evaluated in fp32 in the order written at its entry below, each product and
 * sum rounded once: no fused multiply-add, so a restatement in plain fp32 arithmetic reproduces every element bit for bit.
 * The squares r r are summed in float64, per thread, per block and across blocks in a fixed order: no floating-point atomics,
 * loss_out and gfac_out are bit-identical from run to run.
 *
 * 16-byte accesses are used when the row length (inner; n for the sampler's entry) is a multiple of 4 and every pointer
 * given is 16-byte aligned; a scalar path otherwise.  That is decided per launch.
 */
#ifndef STK_CONSISTENCY_H
#define STK_CONSISTENCY_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* coef is [11, B], row k at coef + k B.  For each of the two levels, with S = (double)sigma[b], d = (double)sigma_data,
 * e = (double)sigma_min, every operation in float64 in this order and the result rounded to fp32 once:
 *   v = S S + d d;  q = sqrt(v);  g = S - e;  w = g g + d d
 *   row 0 / 5  c_in        = 1 / q
 *   row 1 / 6  c_in sigma  = S / q
 *   row 2 / 7  c_skip      = (d d) / w
 *   row 3 / 8  c_out       = (d g) / q
 *   row 4 / 9  c_noise     = log(S) / 4
 * rows 0-4 at sigma_hi, rows 5-9 at sigma_lo, and
 *   row 10     lambda      = 1 / ((double)sigma_hi[b] - (double)sigma_lo[b])
 * One launch of B threads.  The levels are not read back: a non-positive or non-finite level yields NaN or inf in its
 * column, equal levels an infinite lambda.
 * STK_EINVAL: a NULL pointer, B <= 0, sigma_data not positive and finite, sigma_min negative or not finite. */
int stk_ct_coeffs_f32(const float* sigma_hi, const float* sigma_lo, float sigma_data, float sigma_min, float* coef, int B,
                      void* stream);

/* On [B, inner], from one read of y and n (16 B per element):
 *   xin_hi = coef[b] y + coef[B + b] n;  xin_lo = coef[5 B + b] y + coef[6 B + b] n
 * The outputs overlap no operand and not each other.
 * STK_EINVAL: a NULL pointer, B <= 0, inner <= 0.  STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_ct_pair_f32(const float* y, const float* n, const float* coef, float* xin_hi, float* xin_lo, int B, long inner,
                    void* stream);

/* Bytes of the workspace of stk_ct_loss_f32 for B rows of inner floats: the float64 partial sums, one per (sample, block);
 * a function of the two sizes alone, not of the alignment.  Negative where the other entries refuse: STK_EINVAL for B <= 0 or
 * inner <= 0, STK_EUNSUPPORTED for B inner >= 2^31. */
long stk_ct_ws_bytes(int B, long inner);

/* On [B, inner], with sh = sigma_hi[b], sl = sigma_lo[b], and c_skip / c_out of the two levels from coef (rows 2, 3 and 7, 8):
 *   xh = y + sh n;  fh = c_skip_hi xh + c_out_hi F_hi;  xl = y + sl n;  fl = c_skip_lo xl + c_out_lo F_lo;
 *   r = fh - fl;  q = r r
 * The workspace receives, per sample and block, the float64 sum of the block's fp32 q (every slot, every launch: nothing has
 * to be zeroed); a finishing pass enqueued by the same call adds a row's partials in index order within a fixed tree to S and,
 * in float64 with C = (double)c and L = (double)coef[10 B + b], writes
 *   h = sqrt(S + C C);  loss_out[b] = (float)((L S) / (h + C));  gfac_out[b] = (float)((L (double)c_out_hi) / h)
 * both divided by (double)inner before the rounding under reduce_mean.
 * r_out receives r and gfac_out the factor of the gradient; they may be NULL TOGETHER (an evaluation without gradient), and
 * overlap no operand otherwise.
 * ws: at least stk_ct_ws_bytes(B, inner) bytes, 8-byte aligned.
 * STK_EINVAL: a NULL pointer other than r_out and gfac_out, only one of those two NULL, B <= 0, inner <= 0, c not positive and
 * finite, ws_bytes too small, ws misaligned.  STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_ct_loss_f32(const float* F_hi, const float* F_lo, const float* y, const float* n, const float* sigma_hi,
                    const float* sigma_lo, const float* coef, float c, void* ws, long ws_bytes, float* r_out, float* gfac_out,
                    float* loss_out, int B, long inner, int reduce_mean, void* stream);

/* dF = k r on [B, inner] with k = gfac[b] dloss[b] in fp32.  dF may be r itself.
 * STK_EINVAL: a NULL pointer, B <= 0, inner <= 0.  STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_ct_loss_grad_f32(const float* r, const float* gfac, const float* dloss, float* dF, int B, long inner, void* stream);

/* One sampler step on n elements:
 *   x0 = min(max(cs x + co F, lo), hi)                   (lo = -inf, hi = +inf: no clamp; a NaN stays a NaN)
 *   z given:  x_out = x0 + c_z z;  xin_out = c_in_next x_out
 * z NULL (the last step): only x0_out is written, x_out and xin_out are not touched and may be NULL.  x0_out may be NULL where
 * z is given.  x_out may be x, and x0_out may be x where z is NULL or x_out is not x: an item reads everything before it
 * writes, and no two items share an element.  No other overlap.
 * STK_EINVAL: x or F NULL, z given with x_out or xin_out NULL, z NULL with x0_out NULL, n <= 0, lo > hi or either NaN.
 * STK_EUNSUPPORTED: n >= 2^31. */
int stk_ct_step_f32(const float* x, const float* F, const float* z, float cs, float co, float lo, float hi, float c_z,
                    float c_in_next, float* x0_out, float* x_out, float* xin_out, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
