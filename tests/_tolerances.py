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
