/*
 * stk_augment.h -- the non-leaky augmentation of Karras et al. 2022 ("Elucidating the Design Space of Diffusion-Based
 * Generative Models", appendix F.2) for libstk: the geometric operator (flips, then one affine warp between a 2x FIR
 * upsampling and a 2x FIR downsampling) as ONE launch, and the linear embedding of the augmentation labels that is added to
 * the time embedding of the score network, with its gradient.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds the entries only when the library exports them; a network with an
 * augmentation embedding planned on a library without them is refused when it is planned.
 *
 * Conventions are those of stk.h: fp32 tensors on the device, caller-owned outputs, no allocation, no synchronisation,
 * everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise, returned before anything is launched.
 * Arithmetic: fp32, every sum, difference and product rounded once, no fused multiply-add, no atomics: two launches on the
 * same operands give the same bits.
 *
 * ---- The operator, per (sample, channel) plane S[H][W]; pixel i has its centre at i + 1/2 --------------------------------
 * Each sample has a row of 8 floats  (fx, fy, a00, a01, a10, a11, t0, t1):  fx, fy != 0 flip the axis, A = (a00 a01; a10 a11)
 * is the INVERSE linear map (output position -> source position) and t its translation, both in source pixels about the
 * centre c = (W/2, H/2).  x is the W axis, y the H axis.  The low-pass f has T taps, T even, f[k] = f[T-1-k]; h = T / 2.
 *   1. flip     B[y][x] = S[fy ? H-1-y : y][fx ? W-1-x : x],  extended to all integers by reflection without edge repeat:
 *               Bext[i] = B[rho(i, n)],  m = i mod (2n-2) >= 0,  rho = m < n ? m : 2n-2-m           (numpy 'reflect')
 *   2. up 2x    per axis  U[j] = 2 sum_k f[k] Z[j + h - 1 - k],  Z[2i] = Bext[i], Z[odd] = 0; U[j] has its centre at
 *               (j + 1/2) / 2.  The W axis first, then the H axis; the sum over k ascending, the taps that meet a zero of Z
 *               left out, the doubling last (exact).
 *   3. warp     for q on the 2x grid  p = ((qx + 1/2)/2, (qy + 1/2)/2),  u = A (p - c) + c + t,  s = 2u - 1/2, and V[q] the
 *               bilinear interpolation of U at s, U taken on the whole integer lattice:
 *               V = (w00 U[y0][x0] + w01 U[y0][x0+1]) + (w10 U[y0+1][x0] + w11 U[y0+1][x0+1]),  x0 = floor(sx),
 *               gx = sx - x0, w00 = (1-gy)(1-gx), w01 = (1-gy) gx, w10 = gy (1-gx), w11 = gy gx.
 *               ux = ((a00 dx + a01 dy) + cx) + t0', uy likewise, with (dx, dy) = p - c (exact) and t' the translation
 *               reduced by whole periods of U into [-(n-1), n-1] (exact in fp32, see below).
 *   4. down 2x  per axis  O[i] = sum_k f[k] V[2i + k - (h - 1)], k ascending; the W axis first, then the H axis.
 *   5. exact    a row with A = I and t = 0 exactly gives O = B bit for bit: nothing is filtered.  (The branch is taken per
 *               workgroup: one workgroup works on one plane.)
 *
 * The lattice of U.  Bext is even about 0 and about n-1, so Z is even about 0 and about 2(n-1) and has the period
 * Q = 4(n-1).  With a symmetric f, substituting k -> T-1-k in the sum of step 2 gives U[1 - j] = U[j]: U is even about
 * j = 1/2 (the centre of pixel 0 on the 2x lattice), and, from the other mirror of Z, about Q/2 + 1/2.  Every U[j] is
 * therefore one of the 2n values U[0 .. 2n-1], through
 *               sigma(j, n):  m = j mod Q >= 0;  sigma = m < 2n ? m : Q + 1 - m          (Q + 1 - m lies in [2, 2n-3])
 * and the kernel keeps just those 2H x 2W values, however far the warp reaches.  U also has the period Q in s, that is
 * 2(n-1) in u: the kernel replaces t by fmodf(t, 2(n-1)), less one period when that is above n-1 or plus one when it is below
 * -(n-1) -- both steps are exact in fp32 -- so the sampling coordinate, and with it its rounding error, stays small for any
 * translation.  A coordinate that is not finite, or beyond 2^30, is clamped to +-2^30: no entry reads outside its operands
 * whatever the parameters hold.
 *
 * One workgroup per plane keeps B (H W floats), U (4 H W) and V on its (2H + T - 2) x (2W + T - 2) grid in LDS: 154 KB at
 * H = W = 64, T = 12, of the 160 KB of a gfx950 CU.  The row pass of step 2 is staged in the region of V and that of step 4
 * in the region of U.
 */
#ifndef STK_AUGMENT_H
#define STK_AUGMENT_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when stk_aug_warp_f32 takes planes of H x W with T taps: H, W even and in [8, 64], T even and in [2, 12]; else 0. */
int stk_aug_ok(int H, int W, int T);

/* y = the operator above applied to x, both [B, C, H, W]; params [B, 8] on the device; f: T taps on the HOST (read before
 * the launch, passed by value).  y must not overlap x.
 * STK_EINVAL: a NULL pointer, B <= 0, C <= 0, H <= 0, W <= 0, T <= 0, a tap that is not finite.
 * STK_EUNSUPPORTED: !stk_aug_ok(H, W, T), f[k] != f[T-1-k] for some k, B C >= 2^31. */
int stk_aug_warp_f32(const float* x, const float* params, const float* f, int T, float* y, int B, int C, int H, int W,
                     void* stream);

/* y[b][j] = t[b][j] + sum_k labels[b][k] Wt[j][k] on [B, D], labels [B, K], Wt [D, K]: acc = labels[b][0] Wt[j][0], then
 * acc += labels[b][k] Wt[j][k] for k = 1 .. K-1, then y = t + acc; every operation rounded once.  y may be t itself.
 * STK_EINVAL: a NULL pointer, B <= 0, K <= 0, D <= 0.  STK_EUNSUPPORTED: B D >= 2^31, D K >= 2^31 or B K >= 2^31. */
int stk_aug_embed_fwd_f32(const float* t, const float* labels, const float* Wt, float* y, int B, int K, int D, void* stream);

/* gt = gy (beta == 0: an exact copy, gt is not read) or gt + gy (beta == 1) on [B, D], and
 * gWt[j][k] = ((gWt[j][k] + labels[0][k] gy[0][j]) + labels[1][k] gy[1][j]) + ...  over b ascending, one thread per (j, k).
 * gt may be NULL (the gradient of t is not wanted) and gWt may be NULL (the weight's is not: the input-only backward), not
 * both.  gt and gWt overlap neither gy nor each other.
 * STK_EINVAL: gy or labels NULL, gt and gWt both NULL, beta neither 0 nor 1, B <= 0, K <= 0, D <= 0.
 * STK_EUNSUPPORTED: B D >= 2^31, D K >= 2^31 or B K >= 2^31. */
int stk_aug_embed_bwd_f32(const float* gy, const float* labels, float* gt, float beta, float* gWt, int B, int K, int D,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif
