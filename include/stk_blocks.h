/*
 * stk_blocks.h -- entries of libstk that only the stand-alone building blocks need (models/layerspp.py called on their own):
 * gradients the score network never asks for.
 *
 * Only the product library (soft-truncation_amd/csrc -> libstk.so) implements this header; the plain-C checker
 * (oracle/stk_ref.c) does not.  A caller binds these entries only when the library exports them; a graph that needs one
 * on a library without it is refused at planning time, never evaluated some other way.
 */
#ifndef STK_BLOCKS_H
#define STK_BLOCKS_H

#include "stk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Input gradient of the Gaussian Fourier features (stk_fourier_embedding_f32) from the forward's output y = [sin p | cos p],
 * p = x_b W_j 2 pi: a GaussianFourierProjection called on its own may get an input that needs a gradient; the network's
 * noise level never does.
 *   dx[b] = beta dx[b] + 2 pi sum_j W_j (dy[b,j] y[b,nf+j] - dy[b,nf+j] y[b,j])      (beta == 0: dx is not read)
 * One workgroup per sample. */
int stk_fourier_embedding_bwd_f32(const float* W, const float* y, const float* dy, float* dx, float beta, int B, int nf,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif
