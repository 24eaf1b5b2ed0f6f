/*
 * stk_parallel.h -- the three launches of one iteration of the parallel-in-time sampler of libstk (Shih et al., "Parallel
 * Sampling of Diffusion Models", 2023: Picard iteration over a sliding window of grid points): the prefix sum of the window's
 * step increments with the per-slot change norms, the stride decision, and the slide of the window.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a sampler that needs them on
 * a library without them is refused when it is built, never evaluated some other way.
 *
 * Conventions are those of stk.h: tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 *
 * The state is X[W + 1, B, n]: W + 1 slots (slot-major) of B samples, rows of n = C H W contiguous floats.  Slot j holds the
 * current iterate at grid point i0 + j; X[0] is committed.  Of the W slots p = min(W, N - i0) are live, the rest padding.
 * With the step map x_{i+1} = a_i x_i + b_i score(x_i, t_i) + g_i z_i and the device table coef[N, 3] of fp32 rows
 * (a_i - 1, b_i, g_i), one iteration is
 *
 *   S = score(X[0 .. W-1])                                          the caller's, one batch of W B samples
 *   D_j = (coef[i0+j,0] X[j] + coef[i0+j,1] S[j]) + coef[i0+j,2] Z[(i0+j) mod W]
 *   Y[0] = X[0];  Y[j+1] = Y[j] + D_j  (j < p);  err[b][j] = sum over the row of (Y[j] - X[j])^2  (1 <= j < p);
 *   X[1 .. p] <- Y[1 .. p]                                          stk_picard_scan_f32
 *   slot j is converged iff err[b][j] <= thr[i0+j] for every b;  stride = 1 + the leading converged slots of j = 1 .. p-1
 *                                                                   stk_picard_stride
 *   X[j] <- X[min(j + stride, p)], j = 0 .. W                       stk_picard_slide_f32
 *
 * and the caller advances i0 by the stride.  Z[W, B, n] is a ring: the noise of step i lives in slot i mod W.
 *
 * Arithmetic.  D_j and the sums Y[j] + D_j are evaluated in fp32 in the order written, each product and each sum rounded
 * once: no fused multiply-add, and the sums along j strictly sequential, so a restatement in plain fp32 arithmetic reproduces
 * every Y[j] bit for bit -- and with every threshold 0 the iteration reproduces the sequential loop bit for bit.  Each
 * (Y[j] - X[j])^2 is an fp32 difference squared in fp32; the squares are summed in float64, per thread, per wave, per block
 * and across blocks in a fixed order: no floating-point atomics, err is bit-identical from run to run.
 *
 * 16-byte accesses are used when n is a multiple of 4 and every pointer given is 16-byte aligned (then every row starts
 * aligned); a scalar path otherwise.  That is decided per launch.
 *
 * Every entry refuses, before any launch: STK_EINVAL for W < 1, B <= 0 or n <= 0; STK_EUNSUPPORTED for W > 256 or
 * (W + 1) B n >= 2^31 (the index arithmetic is 32-bit); then STK_EINVAL for what is listed with the entry.
 */
#ifndef STK_PARALLEL_H
#define STK_PARALLEL_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of stk_picard_scan_f32 / stk_picard_stride for a window of W slots of B rows of n floats: the
 * float64 partial sums [B, W, blocks per row]; a function of the three sizes alone, not of the alignment.  Negative where the
 * other entries refuse the sizes. */
long stk_picard_ws_bytes(int W, int B, long n);

/* Step 2 above, in place: X[1 .. p] <- Y[1 .. p]; X[0] and the slots beyond p are not written.  S: [W, B, n], slots j >= p
 * are not read.  Z: [W, B, n] or NULL: the g-term is then left out (coef[.,2] and Z are not read).  coef: rows i0 .. i0+p-1
 * of the [N, 3] table are read: the caller keeps i0 + p <= N.  The workspace receives, per sample, slot and block, the
 * float64 sum of the block's fp32 squares (every entry, every launch: nothing has to be zeroed; the entries of slot 0 and
 * of slots >= p are zero).  ws: at least stk_picard_ws_bytes(W, B, n) bytes, 8-byte aligned.  S and Z overlap X nowhere.
 * STK_EINVAL: X, S, coef or ws NULL, p outside [1, W], i0 < 0, ws_bytes too small, ws misaligned. */
int stk_picard_scan_f32(float* X, const float* S, const float* Z, const float* coef, int i0, int p, int W, void* ws,
                        long ws_bytes, int B, long n, void* stream);

/* Step 3, from the workspace stk_picard_scan_f32 left (same W, B, n, p): err[b][j] = the partials of (b, j) summed in index
 * order; thr: the float64 device table [N] of thresholds, entries i0+1 .. i0+p-1 are read.  A NaN err is not converged.
 * stride_out: one int on the device, 1 <= stride <= p.  err_out: NULL, or [W] float64 on the device: the largest err[b][j]
 * over b (NaN if any is), 0 for j = 0 and j >= p.  One block.
 * STK_EINVAL: ws, thr or stride_out NULL, p outside [1, W], i0 < 0, ws_bytes too small, ws misaligned. */
int stk_picard_stride(const void* ws, long ws_bytes, const double* thr, int i0, int p, int W, int B, long n,
                      int* stride_out, double* err_out, void* stream);

/* Step 4, in place: with s = the int at stride_dev clamped to [1, p], X[j] <- X[min(j + s, p)] for j = 0 .. W: the window
 * moves s points on, and the slots that enter it start from the last point computed.
 * STK_EINVAL: X or stride_dev NULL, p outside [1, W]. */
int stk_picard_slide_f32(float* X, const int* stride_dev, int p, int W, int B, long n, void* stream);

#ifdef __cplusplus
}
#endif

#endif
