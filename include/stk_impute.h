/*
 * stk_impute.h -- the data-consistency step of the conditional predictor-corrector samplers of libstk (inpainting and
 * colourisation, score_sde's controllable_generation.py): after a predictor or corrector update the known part of the
 * state is replaced by the data perturbed to the current noise level, in one streaming pass.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entry only when the library exports it; a sampler that needs it on a
 * library without it is refused when it is built, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise.
 *
 * For image n, pixel p, the channel vector x_p = x[n,:,p] and the mask value m (per decoupled channel):
 *   u      = x_p M                (u_j = sum_i x_i M[i][j];  M = mix, row-major;  the identity when mix == NULL)
 *   d      = data_p M
 *   mean_k = a[n] d
 *   known  = mean_k + s[n] z_p    (z lives in the mixed space;  z == NULL: known = mean_k)
 *   v      = u (1 - m) + known m
 *   x_out  = v U                  (U = unmix, row-major;  the identity when unmix == NULL)
 *   xmean  = (v (1 - m) + mean_k m) U
 * The blend is arithmetic, so a mask may hold any value in [0, 1].  With the identity mix and finite operands, x_out is
 * bit-identical to x where m == 0 and does not depend on x where m == 1.
 */
#ifndef STK_IMPUTE_H
#define STK_IMPUTE_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x, data, z, x_out, xmean_out: [N,C,HW].  mask: [mask_n,mask_c,HW] with mask_n in {1,N} and mask_c in {1,C}.  a, s: [N] on
 * the device.  mix, unmix: nine floats each on the HOST (copied into the launch), both given or both NULL.  z and xmean_out may
 * be NULL (no noise term / not written).  x_out may be x itself; no other overlap of an output with an operand is allowed.
 * STK_EUNSUPPORTED, with nothing written: mix given and C != 3, mask_n or mask_c outside their two values, a tensor of 2^31
 * elements or more. */
int stk_impute_f32(const float* x, const float* data, const float* z, const float* mask, const float* a, const float* s,
                   const float* mix, const float* unmix, float* x_out, float* xmean_out, int N, int C, long HW, int mask_n,
                   int mask_c, void* stream);

#ifdef __cplusplus
}
#endif

#endif
