/*
 * stk_adagn.h -- GroupNorm whose affine part is modulated per sample by a conditioning vector ("scale-shift norm": ADM's
 * use_scale_shift_norm, Dhariwal & Nichol, "Diffusion Models Beat GANs on Image Synthesis", 2021; the conditional
 * normalisation of BigGAN), followed by the activation and dropout of stk_gn_fwd_f32.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a network with the
 * modulated layer planned on a library without them is refused when it is planned, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * Definition, x [N, C, HW] (one source), G groups of C / G channels, biased variance:
 *     xhat = (x - mean_ng) rstd_ng ;  u = gamma_c xhat + beta_c ;  v = u (1 + s_nc) + b_nc ;  y = dropout(act(v))
 *     s_nc = mod[n mod_stride + c] ,  b_nc = mod[n mod_stride + C + c]            (scale first, shift second)
 * `mod` points into a row-major matrix of mod_stride >= 2 C columns (the stacked projection of the conditioning vector, at
 * this layer's columns).  Per sample the layer IS a GroupNorm with the affine pair
 *     gamma'_nc = gamma_c (1 + s_nc) ,  beta'_nc = beta_c (1 + s_nc) + b_nc ,
 * and that is how it is evaluated: the kernels are those of stk_gn_fwd_f32 / stk_gn_bwd_f32 with (gamma', beta') formed per
 * (sample, channel) where they load (gamma, beta) -- the same statistics (mean / rstd are bit-equal to the plain entry's
 * whatever the modulation), the same routes by shape and alignment (register-resident, looping, split over `ws` for groups
 * above 16384 elements; 16-byte accesses when HW % 4 == 0 and x, y / dy, dx are 16-byte aligned, scalar ones otherwise),
 * the same `act` codes 0..4 and the same dropout mask, keep(seed + *seed_dev, flat index) of stk_rng.h.  With s = b = 0 the
 * output is bit-equal to stk_gn_fwd_f32's.  `mod` and `dmod` need no alignment.
 *
 * Every float sum is taken in a fixed order and no float atomic is used: two launches on the same operands give the same
 * bits.
 */
#ifndef STK_ADAGN_H
#define STK_ADAGN_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the entries below take the shape (C > 0, HW > 0, G > 0, C % G == 0), else 0. */
int stk_gn_mod_ok(int C, int HW, int G);

/* Bytes of `ws` for either direction: = stk_gn_ws_bytes(N, C, HW, G).  0 for a shape stk_gn_mod_ok refuses. */
long stk_gn_mod_ws_bytes(int N, int C, int HW, int G);

/* Forward.  mean, rstd [N G] are written for the backward.  ws may be NULL: groups too large for one workgroup then take
 * the looping kernel instead of the split route.
 * STK_EINVAL: x, gamma, beta, mod, y, mean or rstd NULL; N, C, HW or G <= 0; C % G != 0; mod_stride < 2 C; act outside
 * 0..4; drop_p outside [0, 1). */
int stk_gn_mod_fwd_f32(const float* x, const float* gamma, const float* beta, const float* mod, int mod_stride, float* y,
                       float* mean, float* rstd, int N, int C, int HW, int G, float eps, int act, float drop_p,
                       unsigned long long seed, const unsigned long long* seed_dev, float* ws, void* stream);

/* Backward, with dv = d(loss)/dv of the definition above (dy through the dropout mask and the activation's slope):
 *     dbeta'_nc = sum_hw dv ,  dgamma'_nc = sum_hw dv xhat                      (left in ws[n][c][0], ws[n][c][1])
 *     dx        = dx_beta dx + rstd (dv gamma' - mean_g(dv gamma') - xhat mean_g(dv gamma' xhat))     (dx_beta 0: dx is not read)
 *     dmod[n mod_stride + c]     = dgamma'_nc gamma_c + dbeta'_nc beta_c        WRITTEN, in the layout of `mod`;
 *     dmod[n mod_stride + C + c] = dbeta'_nc                                    columns outside these 2 C are not touched
 *     dgamma[c] += sum_n dgamma'_nc (1 + s_nc) ,  dbeta[c] += sum_n dbeta'_nc (1 + s_nc)              (n ascending in 8 runs)
 * dx, dmod, dgamma and dbeta may each be NULL (dgamma and dbeta: the input-only backward; dmod too where nothing
 * differentiable feeds `mod`).  ws is required.
 * STK_EINVAL: as the forward, with dy, mean, rstd, ws in place of y. */
int stk_gn_mod_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta, const float* mod, int mod_stride,
                       const float* mean, const float* rstd, float* dx, float dx_beta, float* dmod, float* dgamma, float* dbeta,
                       float* ws, int N, int C, int HW, int G, int act, float drop_p, unsigned long long seed,
                       const unsigned long long* seed_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif
