/*
 * stk_fp16.h -- the fp16 mode of libstk: one-product twins of the forward convolution entries of stk.h.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them, and a caller that asks
 * for the fp16 mode from a library without them gets an error, never the fp32 entries in their place.
 *
 * Contract.  Each twin takes exactly the arguments of its fp32 entry and writes the same output, with the convolution
 * sum replaced by
 *     the fp32-accumulated sum of products of the fp16 `hi` splits of both operands,
 * hi(x) = fp16_rn(x * 2^ex) / 2^ex and hi(w) = fp16_rn(w * 2^ew) / 2^ew, with the per-tensor power-of-two scales the fp32
 * entry uses (the scale record of the activations, the header of the prepared weights); bias, time embedding, residual
 * and out_div are applied as in the fp32 entry.  Error against the fp32 product of the inputs: at most
 * (2u + u^2) (|w| * |x|) + the fp32 accumulation term, u = 2^-11, where |w| * |x| is the convolution of the magnitudes.
 * On shapes whose forward is not a split form (thin-side streaming kernels, the f32-input MFMA tiles, stride 2) a twin
 * returns the same result as its fp32 entry, bit for bit.
 *
 * The twins leave nothing a backward could reuse beyond what the fp32 entries leave (the |x| records of
 * stk_conv2d_fwd_wp_f16x1 are the same).  The data- and weight-gradient twins of the fp16 training mode are declared in
 * stk_fp16_train.h.
 */
#ifndef STK_FP16_H
#define STK_FP16_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one-product twin of stk_conv2d_fwd_pl_f32 (x as planes: only the hi plane is read) */
int stk_conv2d_fwd_pl_f16x1(const void* xpl, const float* xamax, int C, const float* w, int w_layout, const float* bias,
                            const float* temb, int temb_stride, const float* res, float out_div, float* y, int N, int H,
                            int W, int Cout, int KH, int KW, const void* wp, void* ws, long ws_bytes, void* stream);
/* one-product twin of stk_conv2d_fwd_rec_f32 (|x1| / |x2| scale records already in amax) */
int stk_conv2d_fwd_rec_f16x1(const float* x1, int C1, const float* x2, int C2, const float* w, int w_layout,
                             const float* bias, const float* temb, int temb_stride, const float* res, float out_div,
                             float* y, int N, int H, int W, int Cout, int OH, int OW, int KH, int KW, int stride, int pad,
                             const void* wp, float* amax, void* ws, long ws_bytes, void* stream);
/* one-product twin of stk_conv2d_fwd_wp_f32 */
int stk_conv2d_fwd_wp_f16x1(const float* x1, int C1, const float* x2, int C2, const float* w, int w_layout,
                            const float* bias, const float* temb, int temb_stride, const float* res, float out_div,
                            float* y, int N, int H, int W, int Cout, int OH, int OW, int KH, int KW, int stride, int pad,
                            const void* wp, float* amax, void* ws, long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
