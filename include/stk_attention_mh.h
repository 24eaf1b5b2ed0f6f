/*
 * stk_attention_mh.h -- the attention core of AttnBlockpp with several heads: `heads` independent attentions over the
 * contiguous channel slices [n d, (n + 1) d), d = C / heads, of q, k, v, o of shape [B, C, T] viewed as [B, heads, d, T],
 *   s[b,n,t,t'] = scale * sum_c q[b,n,c,t] k[b,n,c,t']          (scale = d^-0.5 in AttnBlockpp)
 *   o[b,n,c,t]  = sum_t' softmax_t'(s[b,n,t,.])[t'] v[b,n,c,t'],
 *   lse[b,n,t]  = log sum_t' exp(s[b,n,t,t']),
 * forward and backward, on the kernels of stk_attention_* (include/stk.h, T <= 256) and of stk_attention_long_*
 * (include/stk_attention_long.h, above) with a workgroup index of (image, head) in place of the image: head (b, n) of an
 * operand sits at b * bstride + n * d * T floats, its lse / delta row at (b * heads + n) * T.  One launch covers all heads.
 * With heads == 1 the entries run the single-head kernels themselves and return their bits.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them and otherwise plans the
 * GEMM + softmax form with a host loop over the heads.
 *
 * Conventions as in stk_attention_long.h: no entry allocates or synchronises, every launch goes to `stream`, an unsupported
 * shape, stride or alignment returns STK_EUNSUPPORTED, a null pointer, a non-positive size, a C that `heads` does not divide
 * or a workspace smaller than stk_attention_mh_ws_bytes says returns STK_EINVAL.  Results are deterministic: every output
 * element has one owning workgroup, nothing is accumulated with atomics.
 *
 * Arithmetic: that of the single-head entries.  Every product is an fp32 product on the fp16 matrix pipe from two-way split
 * operands; the power-of-two scale is ONE per tensor, over all heads (the same |x| pass, the same 4 x 256 scale records).
 *
 * Shapes: C % heads == 0; d = C / heads with d % 32 == 0 and 32 <= d <= 256 (C itself may exceed 256); 4 <= T <= 16384,
 * T % 4 == 0; fewer than 2^31 elements (T <= 256: bytes) per [B, C, T] tensor and its strided extent.  T <= 256 runs the
 * short form, longer sequences the streaming form.
 *
 * Arguments (both directions):
 *   q, k, v      [B, C, T] fp32, 16-byte aligned; image b of each at b * qkv_bstride floats from its pointer, head n of it
 *                n * d * T floats further
 *   qkv_bstride  floats between consecutive images of q, k, v: C*T for separate tensors, 3*C*T for the channel slices of
 *                one stacked [B, 3C, T] projection; a multiple of 4 and >= C*T
 *   o            [B, C, T] contiguous: the attention output (forward: written; backward: read by the streaming form)
 *   lse          [B, heads, T] (forward: written; backward: read, 16-byte aligned)
 *   rec          4 x 256 floats owned by the caller: scale records of q, k, v (written by the forward, read by the backward:
 *                q, k, v must not change between the two calls) and of d_o (written by the backward)
 *   B, C, T      images, channels (all heads together), positions
 *   heads        number of heads
 *   scale        score scale
 *   ws, ws_bytes caller-provided device workspace of at least stk_attention_mh_ws_bytes(B, C, T, heads) bytes, 16-byte
 *                aligned (the streaming form's fp16 planes; the short form needs none and the query then returns 0, in
 *                which case ws may be NULL).  Its contents are not needed between calls.
 * Backward only:
 *   d_o          [B, C, T] contiguous: gradient of o, 16-byte aligned
 *   delta        [B, heads, T] scratch, 16-byte aligned
 *   dq, dk, dv   gradients, image b at b * grad_bstride floats: dX = beta_X * dX + gradient (beta_X == 0: dX is not
 *                read).  Any of the three may be NULL: that gradient is not wanted.  (The short form computes dk and dv
 *                in one kernel and dq in another; a kernel runs when one of its gradients is wanted and stores only those.)
 *   grad_bstride floats between consecutive images of dq, dk, dv (C*T, or 3*C*T for the slices of one [B, 3C, T] tensor)
 *
 *   stk_attention_mh_ok        1 if the entries take (B, C, T, heads), else 0
 *   stk_attention_mh_ws_bytes  workspace bytes for (B, C, T, heads) (both directions); STK_EINVAL / STK_EUNSUPPORTED for
 *                              shapes the entries refuse
 */
#ifndef STK_ATTENTION_MH_H
#define STK_ATTENTION_MH_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

int stk_attention_mh_ok(int B, int C, int T, int heads);
long stk_attention_mh_ws_bytes(int B, int C, int T, int heads);
int stk_attention_mh_fwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, float* o, float* lse,
                             float* rec, int B, int C, int T, int heads, float scale, void* ws, long ws_bytes,
                             void* stream);
int stk_attention_mh_bwd_f32(const float* q, const float* k, const float* v, long qkv_bstride, const float* o,
                             const float* d_o, const float* lse, float* rec, float* delta, float* dq, float beta_q,
                             float* dk, float beta_k, float* dv, float beta_v, long grad_bstride, int B, int C, int T,
                             int heads, float scale, void* ws, long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
