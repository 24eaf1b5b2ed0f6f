/*
 * stk_solver.h -- the update of the few-step deterministic samplers of libstk (DPM-Solver++ in its data-prediction form:
 * first order, which is DDIM, and the second-order multistep form 2M): after one network evaluation the score becomes a
 * data prediction, the prediction is optionally clamped and extrapolated from the previous one, and the state advances,
 * in one streaming pass.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entry only when the library exports it; a sampler that needs it on a
 * library without it is refused when it is built, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise.
 *
 * Per element, in this order:
 *   d     = cx x + cs score               the data prediction x0 = (x + sigma^2 score) / alpha: cx = 1/alpha, cs = sigma^2/alpha
 *   d     = min(max(d, clip_lo), clip_hi) bounds of -inf / +inf leave a finite d bit-identical
 *   D     = d + g (d - d_prev)            d_prev == NULL: D = d
 *   x_out = A x + B D
 *   d_out = d                             d_out may be NULL
 * The coefficients are host values of the step (the schedule is known before the loop starts): for a step from
 * (alpha, sigma) to (alpha', sigma') with h = log(alpha'/sigma') - log(alpha/sigma), A = sigma'/sigma and
 * B = -alpha' expm1(-h); g = h / (2 h_previous) for a second-order step and 0 for a first-order one.  A = 0, B = 1, g = 0
 * returns the data prediction itself.
 */
#ifndef STK_SOLVER_H
#define STK_SOLVER_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x, score, d_prev, x_out, d_out: n floats each.  d_prev and d_out may be NULL.  x_out may be x itself and d_out may be
 * d_prev itself (state and history kept in place: an item reads all it needs before it writes); no other overlap of an
 * output with an operand or with the other output is allowed.
 * STK_EINVAL: x, score or x_out NULL, n <= 0, g != 0 with d_prev == NULL, clip_lo > clip_hi (or a NaN bound).
 * STK_EUNSUPPORTED, with nothing launched: n >= 2^31. */
int stk_dpm_update_f32(const float* x, const float* score, const float* d_prev, float cx, float cs, float g, float A, float B,
                       float clip_lo, float clip_hi, float* x_out, float* d_out, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
