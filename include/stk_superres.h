/*
 * stk_superres.h -- the data-consistency step of the super-resolution predictor-corrector sampler of libstk: after a
 * predictor or corrector update the r x r block means of the state are replaced by the measured low-resolution image
 * perturbed to the current noise level, in one pass.  It is the colouriser's construction (stk_impute.h) with the
 * orthonormal transform acting on the r^2 pixels of a block instead of the 3 channels of a pixel; the kept coefficient is
 * the block's DC term.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a sampler that needs them on
 * a library without them is refused when it is built, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise.
 *
 * For image n, channel c and the r x r block (by, bx) of the plane, P = r^2:
 *   m_x    = (1/P) * sum of x over the block
 *   mean_k = a[n] * low[n,c,by,bx]
 *   known  = mean_k + (s[n] / r) * z[n,c,by,bx]        (z == NULL: known = mean_k)
 *   x_out  = x + (known  - m_x)     on every pixel of the block
 *   xmean  = x + (mean_k - m_x)
 * The orthonormal DC coefficient of a block is r times its mean, so data noise of standard deviation s is s / r on the
 * mean.  r is a power of two: 1/P and s/r are exact scalings.  Every pixel of a block receives the same m_x, so the other
 * r^2 - 1 coefficients of x are kept up to the rounding of the one addition x + delta.  The sum has a fixed order (no
 * atomics): two calls give the same bits, in place or not.
 */
#ifndef STK_SUPERRES_H
#define STK_SUPERRES_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x, x_out, xmean_out: [N,C,H,W].  low, z: [N,C,H/r,W/r].  a, s: [N] on the device.  z and xmean_out may be NULL (no noise
 * term / not written); with z == NULL x_out and xmean_out are bit-identical.  x_out may be x itself; no other overlap of an
 * output with an operand is allowed.
 * STK_EUNSUPPORTED, with nothing written: r not one of 2, 4, 8, 16; H or W not a multiple of r; a tensor of 2^31 elements
 * or more. */
int stk_superres_f32(const float* x, const float* low, const float* z, const float* a, const float* s, float* x_out,
                     float* xmean_out, int N, int C, int H, int W, int r, void* stream);

/* out[p,by,bx] = the mean of the r x r block (by, bx) of plane p of x.  x: [NC,H,W], out: [NC,H/r,W/r], no overlap.  The
 * sum is the one stk_superres_f32 takes.  STK_EUNSUPPORTED as above. */
int stk_block_mean_f32(const float* x, float* out, long NC, int H, int W, int r, void* stream);

#ifdef __cplusplus
}
#endif

#endif
