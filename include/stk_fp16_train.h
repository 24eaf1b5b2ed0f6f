/*
 * stk_fp16_train.h -- the fp16 training mode of libstk: one-product twins of the backward convolution entries of stk.h.
 * Together with the forward twins of stk_fp16.h they make a whole training step run its split convolutions on one fp16
 * product per multiply-add.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them, and a caller that asks
 * for the fp16 training mode from a library without them gets an error, never the fp32 entries in their place.
 *
 * Contract.  Each twin takes exactly the arguments of its fp32 entry and writes the same output, with the contraction
 * replaced by
 *     the fp32-accumulated sum of products of the fp16 `hi` splits of both operands,
 * hi(v) = fp16_rn(v * 2^e) / 2^e with the per-tensor power-of-two scale the fp32 entry uses for that operand: the scale
 * record of dy (data and weight gradient), of x (weight gradient), the header of the prepared weights (data gradient).
 * alpha, beta, the K-split slab order and the slab reduction are those of the fp32 entry, and so are the scale records
 * the call leaves in amax for the next consumer.  Error against the fp32 product of the inputs: at most
 * (2u + u^2) (|a| * |b|) + the fp32 accumulation term, u = 2^-11, where |a| * |b| is the same contraction of the
 * magnitudes.  Shapes whose contraction is not a split form (thin-side streaming kernels, the f32-input MFMA tiles,
 * stride 2) return the same result as the fp32 entry, bit for bit.
 *
 * The scales put every operand's maximum in [2^13, 2^14), so fp16 neither overflows nor loses more than the subnormal
 * tail below 2^-24 of the scaled maximum: the role of a loss scaler in mixed-precision training, exact and per tensor.
 */
#ifndef STK_FP16_TRAIN_H
#define STK_FP16_TRAIN_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one-product twin of stk_conv2d_dgrad_pl_f32 (dy as planes: only the hi plane is read) */
int stk_conv2d_dgrad_pl_f16x1(const void* dypl, const float* dyamax, const float* w, int w_layout, float* dx1, int C1,
                              float beta1, float* dx2, int C2, float beta2, float alpha, int N, int H, int W, int Cout,
                              int KH, int KW, const void* wp, void* ws, long ws_bytes, void* stream);
/* one-product twin of stk_conv2d_dgrad_rec_f32 (|dy| scale record already in amax[512..768)) */
int stk_conv2d_dgrad_rec_f16x1(const float* dy, const float* w, int w_layout, float* dx1, int C1, float beta1, float* dx2,
                               int C2, float beta2, float alpha, int N, int H, int W, int Cout, int OH, int OW, int KH,
                               int KW, int stride, int pad, const void* wp, float* amax, void* ws, long ws_bytes,
                               void* stream);
/* one-product twin of stk_conv2d_dgrad_wp_f32 */
int stk_conv2d_dgrad_wp_f16x1(const float* dy, const float* w, int w_layout, float* dx1, int C1, float beta1, float* dx2,
                              int C2, float beta2, float alpha, int N, int H, int W, int Cout, int OH, int OW, int KH,
                              int KW, int stride, int pad, const void* wp, float* amax, void* ws, long ws_bytes,
                              void* stream);
/* one-product twin of stk_conv2d_wgrad_pl_f32 (x and dy as planes: only their hi planes are read) */
int stk_conv2d_wgrad_pl_f16x1(const void* xpl, const float* xrec, const void* dypl, const float* dyrec, float* dw,
                              float alpha, float* ws, long ws_bytes, int N, int H, int W, int Cin, int Cout, void* stream);
/* one-product twin of stk_conv2d_wgrad_pl_wgs_f32 */
int stk_conv2d_wgrad_pl_wgs_f16x1(const void* xpl, const float* xrec, const void* dypl, const float* dyrec, float* dw,
                                  float alpha, float* ws, long ws_bytes, int N, int H, int W, int Cin, int Cout, int wgs,
                                  void* stream);
/* one-product twin of stk_conv2d_wgrad_amax_f32 */
int stk_conv2d_wgrad_amax_f16x1(const float* x1, int C1, const float* x2, int C2, const float* dy, float* dw, int w_layout,
                                float alpha, float* ws, long ws_bytes, int N, int H, int W, int Cout, int OH, int OW, int KH,
                                int KW, int stride, int pad, const float* amax, int have, void* stream);

#ifdef __cplusplus
}
#endif

#endif
