"""The f32-operand contractions of csrc/conv.hip against float64, on every launch form.

These are the kernels every layer runs on when it does not qualify for the split path (tests/test_gpu_contractions.py):
the f32-input MFMA kernels (igemm::kernel with its A / B loaders on 64- and 128-wide tiles), wgrad9_kernel<32 | 16 | 8>,
splitk_reduce_kernel, the streaming kernels of conv_thin.h and stk_gemm_f32.  Forward and data-gradient calls pass
ws = NULL, so no shape can take the split path; weight-gradient calls get the workspace stk_conv2d_wgrad_ws_bytes asks
for.  Each case first asserts the kernel family it is meant to reach through stk_conv2d_variant (0 = 64-wide tiles,
1 = 128-wide tiles, 3 = wgrad9, 4 = streaming, never 5: a shape the split path would take with scratch does not belong
here); the loader inside a family follows from the case's K % 8, layout, C2 and OW and is named in the case's comment.
The oracle does not restate the planner, so those assertions only run on the device.

Every overwritten output (y, dx under beta == 0, C under beta == 0) and all scratch start as NaN; outputs with
beta != 0 start from seeded data.  Every launch runs twice and must repeat bit for bit (fixed slab orders).  The
reference is torch in float64 on the fp32 inputs.  Errors are max|got - ref| / max|ref|, printed per case with -s,
bounded by tests/_tolerances.py (F32_*).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _tolerances import F32_DGRAD_RTOL, F32_FWD_RTOL, F32_GEMM_RTOL, F32_WGRAD_RTOL
from _util import call, dev_of, rnd
from test_gpu_contractions import _check, _err, _same, _spread, _sync, _w_oihw, _weights

pytestmark = pytest.mark.gpu

CS, CB, W9, THIN = 0, 1, 3, 4          # stk_conv2d_variant: 64-wide tiles, 128-wide tiles, wgrad9, streaming
DIV = float(np.float32(np.sqrt(2.)))


def _nan(d, *shape):
  return torch.full(shape, float('nan'), device=d)


def _assert_variant(lib, direction, c, want):
  """c = (N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout); device only (the oracle has one form)"""
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout = c
  if lib.is_device:
    got = int(lib.conv2d_variant(direction, C1, C2, N, H, W, Cout, OH, OW, K, K, stride, pad, layout))
    assert got == want and got != 5, (direction, c, got, want)


def _id(c):
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout = c[1:13]
  return (f'v{c[0]}_N{N}_{C1}+{C2}_{H}x{W}_o{Cout}_k{K}s{stride}' + ('_nin' if layout else ''))


def _x_ref(x, H, W, K, stride, pad, OH, OW):
  """the float64 input with explicit zero padding, so that a pad-0 convolution of it is the layer (asymmetric padding
  included: any coordinate outside [0, H) x [0, W) reads as zero)"""
  bottom = (OH - 1) * stride + K - pad - H
  right = (OW - 1) * stride + K - pad - W
  assert bottom >= 0 and right >= 0
  return F.pad(x.double(), (pad, right, pad, bottom))


# ---- forward ----------------------------------------------------------------------------------------------------------
FWD_CASES = [
  # variant, N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout
  (CS, 2, 16, 0, 16, 16, 32, 3, 1, 1, 16, 16, 0),       # AFwdK<CS> + BFwd<CS, 9, false>
  (CS, 2, 7, 0, 12, 10, 24, 3, 1, 1, 12, 10, 0),        # ... K = 63: the tail of the 36-wide k chunk; ragged map
  (CS, 2, 20, 11, 12, 10, 24, 3, 1, 1, 12, 10, 0),      # AFwdK<CS> + BFwd<CS, 9, true>: K tail across the source boundary
  (CS, 2, 512, 0, 8, 8, 32, 3, 1, 1, 8, 8, 0),          # K = 4608, the longest accumulation of a 3x3 layer
  (CB, 24, 23, 0, 32, 32, 128, 3, 1, 1, 32, 32, 0),     # AFwdK<CB> + BFwd<CB, 9, false>: K = 207
  (CB, 24, 12, 11, 32, 32, 128, 3, 1, 1, 32, 32, 0),    # AFwdK<CB> + BFwd<CB, 9, true>
  (CS, 3, 3, 0, 17, 17, 48, 3, 2, 0, 8, 8, 0),          # stride 2, pad 0: K = 27, not streaming (thin kernels are stride 1)
  (CS, 2, 32, 0, 16, 16, 32, 3, 2, 0, 8, 8, 0),         # stride 2 with the asymmetric pad of F.pad(0, 1, 0, 1)
  (CS, 3, 64, 32, 8, 8, 64, 1, 1, 0, 8, 8, 0),          # 1x1 Conv2d, K % 8 == 0: AFwdK<CS> + BFwd<CS, 1, true>
  (CB, 96, 40, 0, 16, 16, 128, 1, 1, 0, 16, 16, 0),     # ... AFwdK<CB> + BFwd<CB, 1, true>
  (CS, 3, 13, 0, 8, 8, 40, 1, 1, 0, 8, 8, 0),           # 1x1 Conv2d, K % 8 != 0: AFwdGen<CS>
  (CS, 3, 9, 4, 8, 8, 40, 1, 1, 0, 8, 8, 0),            # AFwdGen<CS> on a concat
  (CS, 96, 13, 0, 16, 16, 128, 1, 1, 0, 16, 16, 0),     # AFwdGen has no 128-wide form: enough tiles for one stay on 64
  (CS, 5, 40, 0, 4, 4, 56, 1, 1, 0, 4, 4, 1),           # NIN: AFwdNin<CS>, ragged Cout
  (CB, 96, 40, 0, 16, 16, 160, 1, 1, 0, 16, 16, 1),     # NIN: AFwdNin<CB>, ragged Cout
  (CS, 5, 13, 0, 4, 4, 56, 1, 1, 0, 4, 4, 1),           # NIN with a K tail: AFwdNin strides over k, any K is in range
  (THIN, 2, 3, 0, 20, 20, 40, 3, 1, 1, 20, 20, 0),      # thin_in_kernel<9>
  (THIN, 2, 4, 0, 20, 20, 40, 3, 1, 1, 20, 20, 0),      # ... 4-channel side
  (THIN, 2, 1, 0, 8, 8, 24, 3, 1, 1, 8, 8, 0),          # ... 1-channel side
  (THIN, 2, 3, 0, 20, 20, 40, 1, 1, 0, 20, 20, 0),      # thin_in_kernel<1>
  (THIN, 2, 40, 24, 20, 20, 3, 3, 1, 1, 20, 20, 0),     # thin_out_kernel<9> on a concat
  (THIN, 2, 136, 0, 12, 20, 4, 3, 1, 1, 12, 20, 0),     # ... more than 128 input channels: two weight blocks
  (THIN, 2, 40, 0, 8, 8, 2, 1, 1, 0, 8, 8, 0),          # thin_out_kernel<1>
]


def _fwd_launch(lib, x1, x2, w, layout, bias, temb, res, div, c):
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, _ = c
  y = _nan(x1.device, N, Cout, OH, OW)
  tptr, tstride = (temb.data_ptr() + 4 * 8, temb.shape[1]) if temb is not None else (None, 0)
  call(lib, 'conv2d_fwd_f32', x1, C1, x2, C2, w, layout, bias, tptr, tstride, res, div, y, N, H, W, Cout, OH, OW, K, K,
       stride, pad, None, 0)
  return y


@pytest.mark.parametrize('case', FWD_CASES, ids=_id)
def test_forward(hip_lib, case):
  """y with the whole epilogue (bias, a temb column slice of a wider tensor, residual, out_div = sqrt 2) and y without."""
  lib, c = hip_lib, case[1:]
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout = c
  _assert_variant(lib, 0, c, case[0])
  d = dev_of(lib)
  Cin = C1 + C2
  x = rnd(N, Cin, H, W, seed=1)
  w = _weights(Cout, Cin, K, layout, seed=3)
  bias, temb, res = rnd(Cout, seed=4), rnd(N, Cout + 24, seed=5), rnd(N, Cout, OH, OW, seed=6)
  x1 = x[:, :C1].contiguous().to(d)
  x2 = x[:, C1:].contiguous().to(d) if C2 else None
  wd, bd, td, rd = (t.to(d) for t in (w, bias, temb, res))
  runs = [{'y': _fwd_launch(lib, x1, x2, wd, layout, bd, td, rd, DIV, c),
           'y plain': _fwd_launch(lib, x1, x2, wd, layout, None, None, None, 1.0, c)} for _ in range(2)]
  _sync(lib)
  _same(runs, 'forward')
  plain = F.conv2d(_x_ref(x, H, W, K, stride, pad, OH, OW), _w_oihw(w, layout, Cout, Cin, K).double(), stride=stride)
  full = (plain + bias.double()[None, :, None, None] + temb[:, 8:8 + Cout].double()[:, :, None, None] + res.double()) / DIV
  _check(f'fwd {_id(case)}', {'y': _err(runs[0]['y'], full), 'y plain': _err(runs[0]['y plain'], plain)}, F32_FWD_RTOL)


# ---- data gradient ----------------------------------------------------------------------------------------------------
DGRAD_CASES = [
  # variant, N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout      (K of the GEMM = Cout * taps)
  (CS, 2, 16, 0, 16, 16, 32, 3, 1, 1, 16, 16, 0),       # ADgrad9<CS>
  (CS, 2, 24, 0, 12, 10, 7, 3, 1, 1, 12, 10, 0),        # ... Cout = 7: K = 63, the tail of the 36-wide chunk; ragged map
  (CS, 2, 20, 11, 12, 10, 24, 3, 1, 1, 12, 10, 0),      # ... two-source dx, the C1 boundary at row 20
  (CS, 2, 3, 0, 20, 20, 40, 3, 1, 1, 20, 20, 0),        # ... the stem's data gradient: three rows of a 64-row tile
  (CS, 2, 32, 0, 8, 8, 512, 3, 1, 1, 8, 8, 0),          # ... K = 4608
  (CB, 24, 128, 0, 32, 32, 23, 3, 1, 1, 32, 32, 0),     # ADgrad9<CB>, Cout = 23: K = 207
  (CB, 24, 70, 58, 32, 32, 23, 3, 1, 1, 32, 32, 0),     # ... two-source dx, the C1 boundary at row 70
  (CS, 3, 48, 0, 17, 17, 3, 3, 2, 0, 8, 8, 0),          # stride 2, 17 x 17 <- 8 x 8, Cout = 3: K = 27
  (CS, 2, 32, 0, 16, 16, 32, 3, 2, 0, 8, 8, 0),         # stride 2, 16 x 16 <- 8 x 8 (asymmetric pad)
  (CS, 3, 40, 24, 8, 8, 64, 1, 1, 0, 8, 8, 0),          # ADgrad1<CS>, two-source dx, the C1 boundary at row 40
  (CS, 3, 40, 0, 8, 8, 13, 1, 1, 0, 8, 8, 0),           # ADgrad1<CS>, K = 13
  (CB, 96, 128, 0, 16, 16, 40, 1, 1, 0, 16, 16, 0),     # ADgrad1<CB>
  (CS, 5, 40, 0, 4, 4, 56, 1, 1, 0, 4, 4, 1),           # NIN: ADgradNin<CS>
  (CB, 96, 128, 0, 16, 16, 40, 1, 1, 0, 16, 16, 1),     # NIN: ADgradNin<CB>
  (CS, 5, 40, 0, 4, 4, 13, 1, 1, 0, 4, 4, 1),           # NIN, Cout % 8 != 0: ADgradNinGen<CS>
  (CS, 96, 128, 0, 16, 16, 13, 1, 1, 0, 16, 16, 1),     # ADgradNinGen has no 128-wide form
  (THIN, 2, 40, 24, 20, 20, 3, 3, 1, 1, 20, 20, 0),     # thin_in_kernel<9> as the data gradient of a head, two-source dx
  (THIN, 2, 136, 0, 12, 20, 4, 3, 1, 1, 12, 20, 0),     # ... Cout = 4, 136 rows in blocks of 32
  (THIN, 2, 24, 0, 8, 8, 2, 3, 1, 1, 8, 8, 0),          # ... Cout = 2
  (THIN, 2, 40, 0, 8, 8, 2, 1, 1, 0, 8, 8, 0),          # thin_in_kernel<1> as a data gradient
  (THIN, 2, 40, 0, 20, 20, 3, 1, 1, 0, 20, 20, 0),      # ... Cout = 3
]


def _dgrad_launch(lib, dy, w, layout, dx1_0, dx2_0, beta1, beta2, alpha, c):
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, _ = c
  d = dy.device
  # beta == 0: dx is overwritten, never read -- it starts as NaN
  dx1 = dx1_0.clone() if beta1 else _nan(d, N, C1, H, W)
  dx2 = (dx2_0.clone() if beta2 else _nan(d, N, C2, H, W)) if C2 else None
  call(lib, 'conv2d_dgrad_f32', dy, w, layout, dx1, C1, beta1, dx2, C2, beta2, alpha, N, H, W, Cout, OH, OW, K, K, stride,
       pad, None, 0)
  return {'dx1': dx1, 'dx2': dx2} if C2 else {'dx1': dx1}


def _dgrad_ref(dy, w, layout, c, alpha):
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, _ = c
  Hp, Wp = (OH - 1) * stride + K, (OW - 1) * stride + K          # the zero-padded input of _x_ref
  g = torch.nn.grad.conv2d_input((dy.shape[0], C1 + C2, Hp, Wp), _w_oihw(w, layout, Cout, C1 + C2, K).double(), dy.double(),
                                 stride=stride)
  return g[:, :, pad:pad + H, pad:pad + W] * alpha


@pytest.mark.parametrize('case', DGRAD_CASES, ids=_id)
def test_data_gradient(hip_lib, case):
  """alpha = 0.5; two sources: dx1 overwritten (NaN before), dx2 accumulated; one source: once overwritten, once
  accumulated."""
  lib, c = hip_lib, case[1:]
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout = c
  _assert_variant(lib, 1, c, case[0])
  d = dev_of(lib)
  Cin = C1 + C2
  dy = rnd(N, Cout, OH, OW, seed=7)
  w = _weights(Cout, Cin, K, layout, seed=3)
  dx1_0, dx2_0 = rnd(N, C1, H, W, seed=8), (rnd(N, C2, H, W, seed=9) if C2 else None)
  alpha = 0.5
  dyd, wd, a1, a2 = dy.to(d), w.to(d), dx1_0.to(d), (dx2_0.to(d) if C2 else None)
  g = _dgrad_ref(dy, w, layout, c, alpha)
  if C2:
    runs = [_dgrad_launch(lib, dyd, wd, layout, a1, a2, 0.0, 0.75, alpha, c) for _ in range(2)]
    ref = {'dx1': g[:, :C1], 'dx2': g[:, C1:] + 0.75 * dx2_0.double()}
  else:
    runs = []
    for _ in range(2):
      r = _dgrad_launch(lib, dyd, wd, layout, a1, None, 0.0, 0.0, alpha, c)
      r['dx1 acc'] = _dgrad_launch(lib, dyd, wd, layout, a1, None, 0.25, 0.0, alpha, c)['dx1']
      runs.append(r)
    ref = {'dx1': g, 'dx1 acc': g + 0.25 * dx1_0.double()}
  _sync(lib)
  _same(runs, 'data gradient')
  _check(f'dgrad {_id(case)}', {k: _err(runs[0][k], ref[k]) for k in ref}, F32_DGRAD_RTOL)


# ---- a batch spread over 4 decades, per image --------------------------------------------------------------------------
SPREAD_CASES = [
  # variant fwd, variant dgrad, N, Cin, Cout, H      (3x3, stride 1)
  (CS, CS, 6, 16, 32, 16),
  (CB, CS, 24, 23, 128, 32),        # forward on 128-wide tiles
  (CS, CB, 24, 128, 23, 32),        # data gradient on 128-wide tiles
]


@pytest.mark.parametrize('case', SPREAD_CASES, ids=lambda c: f'fwd{c[0]}_dgrad{c[1]}_N{c[2]}_{c[3]}to{c[4]}_{c[5]}x{c[5]}')
def test_spread_operand_per_image(hip_lib, case):
  """Per-image magnitudes over 4 decades.  These kernels multiply plain fp32 values, so each image must be right
  relative to its own maximum at the same bound as the whole tensor."""
  vf, vd, N, C, Cout, H = case
  lib = hip_lib
  c = (N, C, 0, H, H, Cout, 3, 1, 1, H, H, 0)
  _assert_variant(lib, 0, c, vf)
  _assert_variant(lib, 1, c, vd)
  d = dev_of(lib)
  x = rnd(N, C, H, H, seed=11) * _spread(N, 1)
  dy = rnd(N, Cout, H, H, seed=12) * _spread(N, 2)
  w = _weights(Cout, C, 3, 0, seed=13)
  xd, dyd, wd = x.to(d), dy.to(d), w.to(d)
  ys = [{'y': _fwd_launch(lib, xd, None, wd, 0, None, None, None, 1.0, c)} for _ in range(2)]
  dxs = [_dgrad_launch(lib, dyd, wd, 0, None, None, 0.0, 0.0, 1.0, c) for _ in range(2)]
  _sync(lib)
  _same(ys, 'forward')
  _same(dxs, 'data gradient')
  yr = F.conv2d(x.double(), w.double(), padding=1)
  dxr = torch.nn.grad.conv2d_input((N, C, H, H), w.double(), dy.double(), padding=1)
  y, dx = ys[0]['y'].cpu(), dxs[0]['dx1'].cpu()
  _check(f'spread fwd v{vf}_N{N}_{C}to{Cout}_{H}x{H}', {'y': _err(y, yr), 'y per image': max(_err(y[i], yr[i]) for i in range(N))}, F32_FWD_RTOL)
  _check(f'spread dgrad v{vd}_N{N}_{C}from{Cout}_{H}x{H}', {'dx': _err(dx, dxr), 'dx per image': max(_err(dx[i], dxr[i]) for i in range(N))},
         F32_DGRAD_RTOL)


# ---- weight gradient --------------------------------------------------------------------------------------------------
WGRAD_CASES = [
  # variant, N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout
  (W9, 8, 32, 0, 32, 32, 48, 3, 1, 1, 32, 32, 0),       # wgrad9_kernel<32>: 16 K splits
  (W9, 19, 48, 0, 16, 16, 40, 3, 1, 1, 16, 16, 0),      # wgrad9_kernel<16>: 9 splits, the last short; Cin = 48: a ragged tile of 32
  (W9, 32, 32, 0, 8, 8, 40, 3, 1, 1, 8, 8, 0),          # wgrad9_kernel<8>: 4 splits
  (CS, 3, 64, 0, 17, 17, 48, 3, 2, 0, 8, 8, 0),         # AWgrad<CS> + BWgrad<CS, false>, stride 2
  (CS, 2, 32, 0, 16, 16, 32, 3, 2, 0, 8, 8, 0),         # ... stride 2 with the asymmetric pad
  (CS, 2, 20, 12, 12, 10, 24, 3, 1, 1, 12, 10, 0),      # AWgrad<CS> + BWgrad<CS, true>: K = 240, not a multiple of 32
  (CS, 5, 40, 0, 4, 4, 56, 1, 1, 0, 4, 4, 1),           # NIN: the reduce writes dw transposed ([Cin][Cout])
  (CS, 3, 64, 32, 8, 8, 64, 1, 1, 0, 8, 8, 0),          # 1x1 Conv2d on a concat
  (CB, 15, 96, 0, 12, 12, 128, 3, 1, 1, 12, 12, 0),     # AWgrad<CB> + BWgrad<CB, false>: K = 2160, 4 splits, the last short
  (CB, 15, 64, 40, 12, 12, 128, 3, 1, 1, 12, 12, 0),    # AWgrad<CB> + BWgrad<CB, true>
  (THIN, 2, 3, 0, 20, 20, 40, 3, 1, 1, 20, 20, 0),      # thin_wgrad_kernel<9, 3>, stem; H W = 400: the second 256-pixel block ragged
  (THIN, 2, 40, 24, 20, 20, 3, 3, 1, 1, 20, 20, 0),     # thin_wgrad_kernel<9, 3>, head on a concat
  (THIN, 2, 4, 0, 20, 20, 40, 3, 1, 1, 20, 20, 0),      # thin_wgrad_kernel<9, 4> at its full width, stem
  (THIN, 2, 40, 0, 20, 20, 4, 3, 1, 1, 20, 20, 0),      # thin_wgrad_kernel<9, 4> at its full width, head
  (THIN, 2, 42, 0, 12, 20, 2, 3, 1, 1, 12, 20, 0),      # thin_wgrad_kernel<9, 4>, 2-channel head; 42 big channels: a ragged block of 4
  (THIN, 2, 1, 0, 8, 8, 24, 3, 1, 1, 8, 8, 0),          # thin_wgrad_kernel<9, 4>, 1-channel stem
  (THIN, 2, 3, 0, 20, 20, 40, 1, 1, 0, 20, 20, 0),      # thin_wgrad_kernel<1, 4>, stem
  (THIN, 2, 40, 0, 8, 8, 2, 1, 1, 0, 8, 8, 0),          # thin_wgrad_kernel<1, 4>, head
]


@pytest.mark.parametrize('case', WGRAD_CASES, ids=_id)
def test_weight_gradient(hip_lib, case):
  """dw += alpha sum dy x into a seeded dw, the workspace NaN before each launch.  The error is relative to
  max|alpha sum dy x|, not to the accumulated dw."""
  lib, c = hip_lib, case[1:]
  N, C1, C2, H, W, Cout, K, stride, pad, OH, OW, layout = c
  _assert_variant(lib, 2, c, case[0])
  d = dev_of(lib)
  Cin = C1 + C2
  x = rnd(N, Cin, H, W, seed=41)
  dy = rnd(N, Cout, OH, OW, seed=42)
  dw0 = rnd(Cin, Cout, seed=43) if layout else rnd(Cout, Cin, K, K, seed=43)
  alpha = 0.5
  x1 = x[:, :C1].contiguous().to(d)
  x2 = x[:, C1:].contiguous().to(d) if C2 else None
  dyd = dy.to(d)
  nb = int(lib.conv2d_wgrad_ws_bytes(C1, C2, N, Cout, OH, OW, K, K))
  assert nb > 0
  runs = []
  for _ in range(2):
    ws = _nan(d, nb // 4)
    dw = dw0.to(d).clone()
    call(lib, 'conv2d_wgrad_f32', x1, C1, x2, C2, dyd, dw, layout, alpha, ws, nb, N, H, W, Cout, OH, OW, K, K, stride, pad)
    runs.append({'dw': dw.cpu()})
  _sync(lib)
  _same(runs, 'weight gradient')
  g = torch.nn.grad.conv2d_weight(_x_ref(x, H, W, K, stride, pad, OH, OW), (Cout, Cin, K, K), dy.double(), stride=stride) * alpha
  if layout:
    g = g.reshape(Cout, Cin).t()
  got = runs[0]['dw'].double()
  assert torch.isfinite(got).all(), 'non-finite result'
  err = ((got - (dw0.double() + g)).abs().max() / g.abs().max()).item()
  _check(f'wgrad {_id(case)}', {'dw': err}, F32_WGRAD_RTOL)


# ---- stk_gemm_f32 -----------------------------------------------------------------------------------------------------
GEMM_CASES = [
  # M, N, K, batch, a k-contiguous, b k-contiguous, bias mode, beta of the accumulating run
  # 64-wide tiles, K = 40: the four loader pairs (GA<CS, ak> x GB<CS, bk>; a row-chunk loader needs unit k stride, K % 8 == 0)
  (70, 66, 40, 3, True, True, 0, 0.5),
  (70, 66, 40, 3, True, False, 1, 0.5),
  (70, 66, 40, 3, False, True, 2, 0.5),
  (70, 66, 40, 3, False, False, 0, 0.5),
  # K = 33: no row-chunk loader whatever the strides; the k tail of the 32-wide chunk is one element
  (130, 70, 33, 2, True, True, 1, 1.0),
  (130, 70, 33, 2, False, False, 2, 1.0),
  # 128-wide tiles (M, N >= 96 and >= 192 tiles): the four loader pairs
  (128, 128, 40, 192, True, True, 1, 0.5),
  (128, 128, 40, 192, True, False, 2, 0.5),
  (128, 128, 40, 192, False, True, 0, 0.5),
  (128, 128, 40, 192, False, False, 1, 0.5),
  (256, 12288, 40, 1, True, False, 2, 0.25),     # ... one wide matrix
  (160, 200, 33, 96, True, True, 2, 0.5),        # ... K = 33, ragged tiles
  # the shapes of the attention block and the embedding MLP (tests/test_gpu_kernels.py)
  (256, 256, 256, 6, False, False, 0, 0.5),      # S = Q^T K
  (256, 256, 256, 6, True, True, 0, 0.5),        # O = V P^T
  (64, 64, 256, 3, True, False, 0, 0.5),
  (512, 7, 128, 1, True, True, 2, 0.5),          # Linear
  (8, 512, 512, 1, True, True, 2, 0.5),          # temb MLP shape (batch 8)
  (16, 16, 16, 5, False, False, 0, 0.5),         # mid-block attention at 4x4
]


@pytest.mark.parametrize('case', GEMM_CASES, ids=str)
def test_gemm(hip_lib, case):
  """C = alpha A B + bias + beta C with alpha = 0.75: beta = 0 on a NaN C and beta != 0 on a seeded one, each into a
  row-major and a transposed C."""
  M, N, K, batch, akc, bkc, bias_mode, beta = case
  lib = hip_lib
  d = dev_of(lib)
  A = rnd(batch, M, K, seed=1) if akc else rnd(batch, K, M, seed=1)
  B = rnd(batch, N, K, seed=2) if bkc else rnd(batch, K, N, seed=2)
  C0 = rnd(batch, M, N, seed=3)
  bias = rnd(M if bias_mode == 1 else N, seed=4) if bias_mode else None
  sam, sak = (K, 1) if akc else (1, M)
  sbk, sbn = (1, K) if bkc else (N, 1)
  alpha = 0.75
  Ad, Bd, bd = A.to(d), B.to(d), (bias.to(d) if bias_mode else None)
  runs = []
  for _ in range(2):
    o = {}
    for name, bt in (('beta 0', 0.0), ('beta', beta)):
      c = C0.to(d).clone() if bt else _nan(d, batch, M, N)
      call(lib, 'gemm_f32', Ad, sam, sak, M * K, Bd, sbk, sbn, N * K, c, N, 1, M * N, bd, bias_mode, M, N, K, batch, alpha, bt)
      ct = C0.transpose(1, 2).contiguous().to(d) if bt else _nan(d, batch, N, M)       # transposed output (scm = 1)
      call(lib, 'gemm_f32', Ad, sam, sak, M * K, Bd, sbk, sbn, N * K, ct, 1, M, M * N, bd, bias_mode, M, N, K, batch, alpha, bt)
      o[name], o[name + ', C^T'] = c, ct.transpose(1, 2)
    runs.append(o)
  _sync(lib)
  _same(runs, 'gemm')
  Am = A.double() if akc else A.double().transpose(1, 2)
  Bm = B.double().transpose(1, 2) if bkc else B.double()
  ref0 = alpha * (Am @ Bm)
  if bias_mode == 1:
    ref0 += bias.double()[None, :, None]
  elif bias_mode == 2:
    ref0 += bias.double()[None, None, :]
  ref = {'beta 0': ref0, 'beta': ref0 + beta * C0.double()}
  errs = {k: _err(v, ref[k.split(',')[0]]) for k, v in runs[0].items()}
  _check(f'gemm {case}', errs, F32_GEMM_RTOL)
