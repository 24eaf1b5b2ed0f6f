/*
 * stk_upconv.h -- the FIR-upsampling convolution of libstk: StyleGAN2's fused up-convolution, the operation
 * models/up_or_down_sampling.upsample_conv_2d of the reference intends (its body reverses the weights with a slice that
 * PyTorch rejects; "flip both spatial axes" is what it means).  Factor 2, square odd K x K weights, ungrouped.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them; a graph that needs the
 * operation on a library without them is refused at planning time, never evaluated some other way.
 *
 * Conventions are those of stk.h: fp32 NCHW tensors on the device, caller-owned outputs and workspaces, no allocation, no
 * synchronisation, everything enqueued on `stream`; 0 on success, a negative STK_E* code otherwise.
 *
 * The operation, for x [N,Cin,H,W], w [Cout,Cin,K,K], FIR taps fir [KT,KT] (already normalised and scaled):
 *   u[n,co,oy,ox]  = sum_ci sum_kh,kw w[co,ci,kh,kw] z[n,ci,oy+kh-(K-1),ox+kw-(K-1)]       u: (2H-2+K) x (2W-2+K)
 *                    z = x with one zero between samples (z[2i,2j] = x[i,j]); z is never formed: each of the four output
 *                    parities contracts only the taps that meet a sample (4 + 2 + 2 + 1 of the 9 for K = 3)
 *   y[n,co,oy,ox]  = (sum_a,b fir[KT-1-a,KT-1-b] u[n,co,oy+a-pad0,ox+b-pad0] + bias[co] + res[n,co,oy,ox]) / out_div
 *                    y: 2H x 2W, u read as zero outside its range   (upfirdn2d(u, fir, pad=(pad0, pad1)), pad1 implied)
 *   du             = the adjoint of that FIR applied to dy:  du[uy,ux] = sum_a,b fir[a,b] dy[uy+a-(KT-1-pad0), ux+b-(KT-1-pad0)]
 *   dx[n,ci,i,j]   = beta dx + alpha sum_co sum_kh,kw w[co,ci,kh,kw] du[n,co,2i+(K-1)-kh,2j+(K-1)-kw]
 *   dw[co,ci,kh,kw] += alpha sum_n,i,j x[n,ci,i,j] du[n,co,2i+(K-1)-kh,2j+(K-1)-kw]
 *
 * du is a caller-owned buffer of N Cout (2H-2+K) (2W-2+K) floats shared by the two gradient entries: with du_valid == 0 an
 * entry first fills it from dy, with du_valid != 0 it reads what an earlier call left there (dy is then not read).
 */
#ifndef STK_UPCONV_H
#define STK_UPCONV_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of direction dir (0 forward: the map u; 1 data gradient: none; 2 weight gradient: the split-K slabs).
 * < 0: the shape is not supported (K not 1 or 3, KT not in 1..4, a tensor of 2^31 elements or more). */
long stk_upconv2d_ws_bytes(int dir, int N, int H, int W, int Cin, int Cout, int K, int KT);

/* y = (FIR(upconv(x, w)) + bias + res) / out_div.  bias, res may be NULL.  ws: stk_upconv2d_ws_bytes(0, ...) bytes. */
int stk_upconv2d_fwd_f32(const float* x, const float* w, const float* fir, const float* bias, const float* res,
                         float out_div, float* y, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0,
                         void* ws, long ws_bytes, void* stream);

/* dx = beta dx + alpha (dense stride-2 gather of du with w); beta == 0: dx is not read. */
int stk_upconv2d_dgrad_f32(const float* dy, const float* w, const float* fir, float* du, int du_valid, float* dx,
                           float beta, float alpha, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0,
                           void* stream);

/* dw += alpha (...), one GEMM per tap split over the pixels into slabs that a second kernel sums in a fixed order:
 * deterministic.  ws: stk_upconv2d_ws_bytes(2, ...) bytes. */
int stk_upconv2d_wgrad_f32(const float* x, const float* dy, const float* fir, float* du, int du_valid, float* dw,
                           float alpha, int N, int H, int W, int Cin, int Cout, int K, int KT, int pad0, void* ws,
                           long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
