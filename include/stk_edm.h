/*
 * stk_edm.h -- the element-wise work of the EDM formulation of libstk (Karras et al., "Elucidating the Design Space of
 * Diffusion-Based Generative Models", 2022, Table 1 column "Ours" and Algorithm 2): the per-sample coefficients of the
 * preconditioned denoiser, the weighted denoising loss with its gradient, and the launches of the (optionally stochastic)
 * Heun sampler.  The network F runs between these launches; it is the caller's.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a loss or a sampler that
 * needs them on a library without them takes its torch-expression path (the loss) or is refused when it is built (the
 * sampler).
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * With s = sigma_data the denoiser at the noise level sigma is D(x; sigma) = c_skip x + c_out F(c_in x; c_noise),
 *
 *   c_in = 1 / sqrt(sigma^2 + s^2),  c_skip = s^2 / (sigma^2 + s^2),  c_out = sigma s / sqrt(sigma^2 + s^2),
 *   c_noise = ln(sigma) / 4,  and the loss weight lambda = 1 / c_out^2.
 *
 * A training evaluation on B samples y of `inner` = C H W floats, with noise n and levels sigma[B]:
 *
 *   coef           = the six rows below                             stk_edm_coeffs_f32
 *   x_in           = c_in y + (c_in sigma) n                        stk_perturb_f32 of stk.h (a = row 0, s = row 1)
 *   F              = network(x_in, c_noise)                         the caller's
 *   r              = (c_skip (y + sigma n) + c_out F) - y,
 *   loss[b]        = lambda_b sum r^2  (/ inner)                    stk_edm_loss_f32
 *   dF             = (2 lambda_b c_out_b dloss_b (/ inner)) r       stk_edm_loss_grad_f32
 *
 * One step of the sampler from t_i to t_{i+1}, with the churned level t^ >= t_i (Algorithm 2):
 *
 *   x^   = x + c_eps eps,  xin = c_in(t^) x^                        stk_edm_churn_f32 (only where t^ > t_i, and before step 0)
 *   F    = network(xin, c_noise(t^))                                the caller's
 *   d    = (x^ - D(x^; t^)) / t^,  x' = x^ + (t_{i+1} - t^) d       stk_edm_step_f32, the Euler stage
 *   F'   = network(c_in(t_{i+1}) x', c_noise(t_{i+1}))              the caller's, unless t_{i+1} = 0
 *   d'   = (x' - D(x'; t_{i+1})) / t_{i+1},
 *   x    = x^ + (t_{i+1} - t^) (d / 2 + d' / 2)                     stk_edm_step_f32, the correction
 *
 * Arithmetic.  Every element-wise expression is evaluated in fp32 in the order written at its entry below, each product,
 * quotient and sum rounded once: no fused multiply-add, so a restatement in plain fp32 arithmetic reproduces every element
 * bit for bit.  The squares r r are summed in float64, per thread, per block and across blocks in a fixed order: no
 * floating-point atomics, loss_out is bit-identical from run to run.
 *
 * 16-byte accesses are used when the row length (inner; n for the sampler's entries) is a multiple of 4 and every pointer
 * given is 16-byte aligned; a scalar path otherwise.  That is decided per launch.
 */
#ifndef STK_EDM_H
#define STK_EDM_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* coef is [6, B], row k at coef + k B.  With S = (double)sigma[b], d = (double)sigma_data, every operation in float64 in
 * this order and the result rounded to fp32 once:
 *   v = S S + d d;  q = sqrt(v);  p = S d;
 *   row 0  c_in        = 1 / q
 *   row 1  c_in sigma  = S / q
 *   row 2  c_skip      = (d d) / v
 *   row 3  c_out       = p / q
 *   row 4  lambda      = v / (p p)
 *   row 5  c_noise     = log(S) / 4
 * One launch of B threads.  sigma is not read back: a non-positive or non-finite sigma[b] yields NaN or inf in its column.
 * STK_EINVAL: a NULL pointer, B <= 0, sigma_data not positive and finite. */
int stk_edm_coeffs_f32(const float* sigma, float sigma_data, float* coef, int B, void* stream);

/* Bytes of the workspace of stk_edm_loss_f32 for B rows of inner floats: the float64 partial sums, one per (sample, block);
 * a function of the two sizes alone, not of the alignment.  Negative where the other entries refuse: STK_EINVAL for B <= 0 or
 * inner <= 0, STK_EUNSUPPORTED for B inner >= 2^31. */
long stk_edm_ws_bytes(int B, long inner);

/* On [B, inner], with sg = sigma[b], c_skip = coef[2 B + b], c_out = coef[3 B + b], lambda = coef[4 B + b]:
 *   x = y + sg n;  D = c_skip x + c_out F;  r = D - y;  q = r r
 * The workspace receives, per sample and block, the float64 sum of the block's fp32 q (every slot, every launch: nothing has
 * to be zeroed); a finishing pass enqueued by the same call adds a row's partials in index order within a fixed tree to S and
 * writes loss_out[b] = (float)((double)lambda S), or (float)(((double)lambda S) / (double)inner) under reduce_mean.
 * r_out receives r; it may be NULL (an evaluation without gradient), and overlaps no operand otherwise.
 * ws: at least stk_edm_ws_bytes(B, inner) bytes, 8-byte aligned.
 * STK_EINVAL: a NULL pointer other than r_out, B <= 0, inner <= 0, ws_bytes too small, ws misaligned.
 * STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_edm_loss_f32(const float* F, const float* y, const float* n, const float* sigma, const float* coef, void* ws,
                     long ws_bytes, float* r_out, float* loss_out, int B, long inner, int reduce_mean, void* stream);

/* dF = k r on [B, inner] with k = ((2 lambda) c_out) dloss[b] in fp32, and k = k / (float)inner after that under reduce_mean
 * (lambda = coef[4 B + b], c_out = coef[3 B + b]).  dF may be r itself.
 * STK_EINVAL: a NULL pointer, B <= 0, inner <= 0.  STK_EUNSUPPORTED: B inner >= 2^31. */
int stk_edm_loss_grad_f32(const float* r, const float* coef, const float* dloss, float* dF, int B, long inner, int reduce_mean,
                          void* stream);

/* x^ = x + c_eps eps;  xin = c_in_hat x^  on n elements.  eps may be NULL: x^ = x, nothing is added (c_eps must be 0), and
 * x_hat_out may then be NULL as well.  x_hat_out may be x; no other overlap.
 * STK_EINVAL: x or xin_out NULL, x_hat_out NULL with eps given, eps NULL with c_eps != 0, n <= 0, c_eps negative or NaN.
 * STK_EUNSUPPORTED: n >= 2^31. */
int stk_edm_churn_f32(const float* x, const float* eps, float c_eps, float c_in_hat, float* x_hat_out, float* xin_out, long n,
                      void* stream);

/* Both stages of a Heun step, on n elements:
 *   D = cs xe + co F;  dn = (xe - D) / t;  slope = d_prev ? 0.5 d_prev + 0.5 dn : dn;
 *   x_out = xb + h slope;  d_out = dn;  xin_out = c_next x_out
 * Euler stage: xe == xb (read once), d_prev NULL.  Correction: xb = x^, xe = the Euler point, d_prev = the Euler slope.
 * d_out and xin_out may be NULL.  x_out may be xb or xe, and d_out may be d_prev: an item reads everything before it writes,
 * and no two items share an element.  No other overlap.
 * STK_EINVAL: xb, xe, F or x_out NULL, n <= 0, t not positive and finite.  STK_EUNSUPPORTED: n >= 2^31. */
int stk_edm_step_f32(const float* xb, const float* xe, const float* F, const float* d_prev, float cs, float co, float t,
                     float h, float c_next, float* x_out, float* d_out, float* xin_out, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
