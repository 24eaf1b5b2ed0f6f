"""The error bounds of the plane-operand contractions (csrc/conv_x2d.h, csrc/conv_x2w.h), in one place.

Each fp32 product of these kernels is three fp16 MFMAs over the planes of both operands (include/stk.h "Planes"), so a
correct kernel is accurate to the fp32 accumulation level.  The bounds are max|got - ref| / max|ref| against a float64
reference of the same operation on the fp32 inputs (tests/test_gpu_contractions.py), set at about 3x the worst case
measured on an MI355X over every launch form.  tests/test_tolerance_model.py keeps them honest on CPU: a numpy model of
the split lands at <= 1/10 of each bound when correct and >= 5x when one term of the split is wrong.
"""

# worst measured (MI355X, tests/test_gpu_contractions.py): fwd 1.47e-6 (16-wide halo kernel, one image of a batch spread
# over 4 decades), dgrad 1.36e-6 (the same; 1.35e-6 on the two-source 16-wide halo), wgrad 6.8e-7 (w32 at batch 128)
PL_FWD_RTOL = 4.5e-6    # forward, y = (conv(x, w) + bias + temb + res) / out_div
PL_DGRAD_RTOL = 4e-6    # data gradient, dx = beta dx + alpha conv_transpose(dy, w)
PL_WGRAD_RTOL = 2e-6    # weight gradient, relative to max|alpha sum dy x| (not to the dw it accumulates into)

# The f32-operand contractions (csrc/conv.hip: the f32-input MFMA kernels, wgrad9_kernel, the streaming kernels of
# conv_thin.h, stk_gemm_f32): plain fp32 products accumulated in fp32 along K.  Same metric and reference, set at about 3x
# the worst case measured on an MI355X over every case of tests/test_gpu_f32_contractions.py (the per-case table is
# profiles/f32_contraction_accuracy.txt).  Ceilings, from strictly sequential fp32 accumulation at the longest K of those
# cases: 1e-5 for forward / data gradient / GEMM, 2e-5 for the weight gradient.
# worst measured: fwd 2.33e-6 (64-wide tiles, 512 -> 32 at 8 x 8: K = 4608, no epilogue), dgrad 2.73e-6 (the same layer:
# 32 <- 512, K = 4608), wgrad 5.75e-7 (128-wide generic kernel, N15 96 -> 128 at 12 x 12: K = 2160 in 4 slabs),
# gemm 7.08e-7 (256 x 256 x 256, batch 6, both operands strided over k, beta = 0.5).
# Next: a batch spread over 4 decades, 1.98e-6 / 1.61e-6 for its worst image (fwd / dgrad; 1.06e-6 / 1.37e-6 over the whole
# tensor); every other case is below 7e-7.
F32_FWD_RTOL = 7e-6     # forward, y = (conv(x, w) + bias + temb + res) / out_div
F32_DGRAD_RTOL = 8e-6   # data gradient, dx = beta dx + alpha conv_transpose(dy, w)
F32_WGRAD_RTOL = 1.5e-6 # weight gradient, relative to max|alpha sum dy x| (not to the dw it accumulates into)
F32_GEMM_RTOL = 2e-6    # stk_gemm_f32, C = alpha A B + bias + beta C
