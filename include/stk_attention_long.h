/*
 * stk_attention_long.h -- the attention core of AttnBlockpp (models/layerspp.py:95-99) on maps above 16 x 16: a streaming
 * ("online softmax") forward and a FlashAttention-2-shaped backward that never hold a [B, T, T] matrix in memory,
 *   o[b,c,t] = sum_t' softmax_t'( scale * sum_c' q[b,c',t] k[b,c',t'] ) v[b,c,t'],
 *   lse[b,t] = log sum_t' exp( scale * sum_c' q[b,c',t] k[b,c',t'] ),
 * in the arithmetic class of stk_attention_* (include/stk.h): every product is an fp32 product on the fp16 matrix pipe
 * from two-way split operands (power-of-two scale per tensor, hi + lo, three MFMAs, fp32 accumulation).
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them and otherwise plans the
 * GEMM + softmax form; shapes stk_attention_ok takes keep running on the short kernels of include/stk.h.
 *
 * Conventions as in stk.h: no entry allocates or synchronises, every launch goes to `stream`, an unsupported shape,
 * stride or alignment returns STK_EUNSUPPORTED, a null pointer or a non-positive size STK_EINVAL.  Results are
 * deterministic: every output element has one owning workgroup, nothing is accumulated with atomics.
 *
 * Shapes: 32 <= C <= 256, C % 32 == 0, 4 <= T <= 16384, T % 4 == 0, fewer than 2^31 elements per [B, C, T] tensor.
 *
 * Range: a tensor's power-of-two scale is at most 2^127, and so is the scale of a score-gradient column ds; the
 * epilogues undo them one after the other, so dq and dk are right wherever (scale / s_k) / sig (dq) and
 * (scale / s_q) / sig (dk) are fp32 numbers: with |q|, |k|, |v| around 1, down to gradients d_o of 2^-100 and below.  Once
 * that factor is subnormal (s_x sig above scale 2^126) it keeps 2^-149 absolute, and the result degrades gradually.
 * What remains outside: max |q| or max |k| below scale 2^-113 (scale / s_x is then itself subnormal), products
 * s_q s_k or s_v s_do above 2^127 (the scores or dp are then below fp32 range themselves), and entries of ds under
 * 2^-126, which do not contribute.
 *
 * Arguments (both directions):
 *   q, k, v      [B, C, T] fp32, 16-byte aligned; image b of each at b * qkv_bstride floats from its pointer
 *   qkv_bstride  floats between consecutive images of q, k, v: C*T for separate tensors, 3*C*T for the channel slices of
 *                one stacked [B, 3C, T] projection; a multiple of 4 and >= C*T
 *   o            [B, C, T] contiguous: the attention output (forward: written; backward: read, for delta)
 *   lse          [B, T]: log-sum-exp of each query's scaled scores (forward: written; backward: read, 16-byte aligned)
 *   rec          4 x 256 floats owned by the caller: scale records (partial |x| maxima, stk.h "Planes") of q, k, v in
 *                rec[0..768) written by the forward, and of d_o in rec[768..1024) written by the backward; the backward
 *                reads the forward's three, so q, k, v must not change between the two calls
 *   B, C, T      images, channels, positions (T = H*W)
 *   scale        score scale (C^-0.5 in AttnBlockpp)
 *   ws, ws_bytes caller-provided device workspace of at least stk_attention_long_ws_bytes(B, C, T) bytes, 16-byte
 *                aligned: the fp16 planes of q, k, v (and d_o) are written there once per call and read by the kernels.
 *                Its contents are not needed between calls.
 * Backward only:
 *   d_o          [B, C, T] contiguous: gradient of o, 16-byte aligned
 *   delta        [B, T] scratch, 16-byte aligned: sum_c d_o[b,c,t] o[b,c,t] (written, then read by the gradient kernels)
 *   dq, dk, dv   gradients, image b at b * grad_bstride floats: dX = beta_X * dX + gradient (beta_X == 0: dX is not
 *                read).  Any of the three may be NULL: that gradient is not computed (dq) or not stored (dk, dv).
 *   grad_bstride floats between consecutive images of dq, dk, dv (C*T, or 3*C*T for the slices of one [B, 3C, T] tensor)
 *
 *   stk_attention_long_ok        1 if the entries take (B, C, T), else 0
 *   stk_attention_long_ws_bytes  workspace bytes for (B, C, T) (both directions), STK_EUNSUPPORTED for other shapes
 */
#ifndef STK_ATTENTION_LONG_H
#define STK_ATTENTION_LONG_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

int stk_attention_long_ok(int B, int C, int T);
long stk_attention_long_ws_bytes(int B, int C, int T);
int stk_attention_long_fwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, float* o, float* lse,
                               float* rec, int B, int C, int T, float scale, void* ws, long ws_bytes, void* stream);
int stk_attention_long_bwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, const float* o,
                               const float* d_o, const float* lse, float* rec, float* delta, float* dq, float beta_q,
                               float* dk, float beta_k, float* dv, float beta_v, long grad_bstride, int B, int C, int T,
                               float scale, void* ws, long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
