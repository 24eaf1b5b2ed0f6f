"""The one-product backward twins (include/stk_fp16_train.h) on every backward launch form.

Each case first asserts its launch form through the library's plan diagnostics, then:
  - exactness: the result equals the float64 contraction of the fp16 `hi` splits of both operands, at the scales the
    kernel uses (the |dy| / |x| scale records, the |w| maxima of the prepared weights), within fp32 accumulation error;
  - against the fp32 inputs: |r - r64| <= (2u + u^2) (|a| * |b|) + the fp32 term, elementwise, u = 2^-11;
  - repeatability: two launches give identical bits (and prepared weights the same bits as weights prepared in ws);
  - the forms that are not split forms (thin-side, f32-input tiles, stride 2) give the fp32 entry's bits exactly.
Errors are printed per case with -s.  (The helpers of test_gpu_fp16_contractions.py are imported, not changed.)
"""
import numpy as np
import pytest
import torch

from _util import call, rnd
from test_gpu_contractions import _assert_form, _planes, _prepare, _record, _w_oihw, _weights
from test_gpu_fp16_contractions import EXACT_RTOL, FP32_TERM, U, _header_scale, _hi, _pow2_scale_of

pytestmark = pytest.mark.gpu

D = torch.device('cuda:0')


def _report(label, got, exact, r64, mag, scale=None):
  """exactness against the hi * hi float64 result and the elementwise bound against the fp32 inputs; `scale` = the
  magnitude errors are relative to (default max|r64|)"""
  got = got.detach().cpu().double()
  assert torch.isfinite(got).all()
  s = r64.abs().max().item() if scale is None else scale
  e_exact = (got - exact).abs().max().item() / s
  bound = (2 * U + U * U) * mag + FP32_TERM * s
  excess = ((got - r64).abs() - bound).max().item()
  e_fp32 = (got - r64).abs().max().item() / s
  print(f'  {label}: vs hi*hi float64 {e_exact:.2e} (bound {EXACT_RTOL:.0e}), vs fp32 inputs {e_fp32:.2e}, '
        f'elementwise bound slack {-excess:.3e}')
  assert e_exact <= EXACT_RTOL, f'{label}: not the one-product result: {e_exact:.3e}'
  assert excess <= 0, f'{label}: |r - r64| exceeds (2u + u^2)(|a| * |b|) + fp32 term by {excess:.3e}'


def _dgrad64(dy, w, layout, Cin, K, alpha):
  N, Cout, H, W = dy.shape
  return torch.nn.grad.conv2d_input((N, Cin, H, W), _w_oihw(w, layout, Cout, Cin, K).double(), dy.double(),
                                    padding=K // 2) * alpha


# ---- data gradient, dy as planes: stk_conv2d_dgrad_pl_f16x1 ----------------------------------------------------------------
DGRAD_PL_CASES = [
  # form, N, C1, C2, H, W, Cout, K, layout
  ('h16', 24, 256, 256, 16, 16, 256, 3, 0),   # up path at 16 x 16, two outputs
  ('h32', 8, 256, 128, 32, 32, 128, 3, 0),    # up path at 32 x 32: 256 + 128 -> 128
  ('h32', 12, 96, 160, 32, 32, 96, 3, 0),     # 3 channel groups of dy: the last pair's second slot is the zero DMA
  ('h64', 3, 128, 128, 64, 64, 128, 3, 0),
  ('g9', 4, 128, 0, 128, 128, 128, 3, 0),     # un-split 3x3
  ('ks4', 128, 256, 0, 8, 8, 256, 3, 0),      # K split
  ('ks6', 128, 256, 0, 4, 4, 256, 3, 0),
  ('g1', 48, 256, 0, 16, 16, 256, 1, 0),      # 1x1 Conv2d
  ('g1', 128, 256, 0, 16, 16, 256, 1, 1),     # NIN
]


def _dgrad_pl_run(lib, entry, yp, rec, wd, layout, C1, C2, K, dx1_0, dx2_0, beta1, beta2, alpha, wp=None):
  N, H, W = dx1_0.shape[0], dx1_0.shape[2], dx1_0.shape[3]
  Cout = wd.shape[1] if layout == 1 else wd.shape[0]
  fb = max(int(lib.conv2d_dgrad_ws_bytes(C1, C2, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=D)
  dx1 = dx1_0.clone()
  dx2 = dx2_0.clone() if C2 else None
  call(lib, entry, yp, rec, wd, layout, dx1, C1, beta1, dx2, C2, beta2, alpha, N, H, W, Cout, K, K, wp, ws, fb)
  return torch.cat([dx1, dx2], 1) if C2 else dx1


def _dgrad_id(c):
  return f'{c[0]}_N{c[1]}_{c[2]}+{c[3]}from{c[6]}_{c[4]}x{c[5]}_k{c[7]}' + ('_nin' if c[8] else '')


@pytest.mark.parametrize('case', DGRAD_PL_CASES, ids=_dgrad_id)
def test_dgrad_pl_twin(hip_lib, case):
  form, N, C1, C2, H, W, Cout, K, layout = case
  lib = hip_lib
  Cin = C1 + C2
  _assert_form(lib, 1, C1, C2, N, H, W, Cout, K, form)
  dy = rnd(N, Cout, H, W, seed=7)
  w = _weights(Cout, Cin, K, layout, seed=3)
  dx0 = rnd(N, Cin, H, W, seed=8)
  beta1, beta2, alpha = 0.25, 0.75, 0.5
  dyd, wd, dx0d = dy.to(D), w.to(D), dx0.to(D)
  rec = _record(lib, dyd)
  yp = _planes(lib, dyd, rec)
  a1, a2 = dx0d[:, :C1].contiguous(), (dx0d[:, C1:].contiguous() if C2 else None)
  args = (yp, rec, wd, layout, C1, C2, K, a1, a2, beta1, beta2, alpha)
  runs = [_dgrad_pl_run(lib, 'conv2d_dgrad_pl_f16x1', *args) for _ in range(2)]
  blk, wp = _prepare(lib, 1, wd, layout, Cin, Cout, K, (C1, C2, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_dgrad_pl_run(lib, 'conv2d_dgrad_pl_f16x1', *args, wp=wp))
  r32 = _dgrad_pl_run(lib, 'conv2d_dgrad_pl_f32', *args, wp=wp)
  torch.cuda.synchronize()
  for r in runs[1:]:
    assert torch.equal(r, runs[0]), 'fp16 twin: launches / prepared weights differ in bits'
  assert not torch.equal(runs[0], r32), 'the fp16 twin returned the fp32 result'
  sy, sw = _pow2_scale_of(rec.max().item()), _header_scale(blk, wp)
  beta = torch.tensor([beta1] * C1 + [beta2] * C2, dtype=torch.float64)[None, :, None, None]
  acc = beta * dx0.double()
  exact = _dgrad64(_hi(dy, sy), _hi(w, sw), layout, Cin, K, alpha) + acc
  r64 = _dgrad64(dy, w, layout, Cin, K, alpha) + acc
  mag = _dgrad64(dy.abs(), w.abs(), layout, Cin, K, alpha)
  _report(f'dgrad pl {_dgrad_id(case)}', runs[0], exact, r64, mag, scale=(r64 - acc).abs().max().item())


# ---- data gradient, dy in fp32 (split in the loader): stk_conv2d_dgrad_wp_f16x1 / _rec_f16x1 -------------------------------
DGRAD_X2_CASES = [
  # N, C1, C2, H, W, Cout, K, layout
  (128, 256, 0, 16, 16, 256, 1, 1),           # NIN shortcut
  (48, 256, 128, 16, 16, 256, 1, 0),          # the up path's 1x1 shortcut over a concat: two outputs
  (24, 256, 128, 16, 16, 256, 3, 0),          # a 3x3 over a concat
]


def _dgrad_x2_run(lib, entry, dyd, wd, layout, C1, C2, K, dx0d, amax, wp=None):
  N, Cout, H, W = dyd.shape
  fb = max(int(lib.conv2d_dgrad_ws_bytes(C1, C2, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=D)
  dx1 = dx0d[:, :C1].clone()                        # (a copy also when C2 = 0: dx0d is every run's starting point)
  dx2 = dx0d[:, C1:].clone() if C2 else None
  call(lib, entry, dyd, wd, layout, dx1, C1, 0.25, dx2, C2, 0.75, 0.5, N, H, W, Cout, H, W, K, K, 1, K // 2, wp, amax, ws, fb)
  return torch.cat([dx1, dx2], 1) if C2 else dx1


@pytest.mark.parametrize('case', DGRAD_X2_CASES, ids=lambda c: f'N{c[0]}_{c[1]}+{c[2]}from{c[5]}_{c[3]}x{c[4]}_k{c[6]}')
def test_dgrad_fp32_operand_twin(hip_lib, case):
  N, C1, C2, H, W, Cout, K, layout = case
  lib = hip_lib
  Cin = C1 + C2
  assert int(lib.conv2d_variant(1, C1, C2, N, H, W, Cout, H, W, K, K, 1, K // 2, layout)) == 5      # the x2 split form
  dy = rnd(N, Cout, H, W, seed=7)
  w = _weights(Cout, Cin, K, layout, seed=3)
  dx0 = rnd(N, Cin, H, W, seed=8)
  dyd, wd, dx0d = dy.to(D), w.to(D), dx0.to(D)
  amax = torch.zeros(768, device=D)
  args = (dyd, wd, layout, C1, C2, K, dx0d, amax)
  runs = [_dgrad_x2_run(lib, 'conv2d_dgrad_wp_f16x1', *args) for _ in range(2)]
  blk, wp = _prepare(lib, 1, wd, layout, Cin, Cout, K, (C1, C2, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_dgrad_x2_run(lib, 'conv2d_dgrad_wp_f16x1', *args, wp=wp))
  runs.append(_dgrad_x2_run(lib, 'conv2d_dgrad_rec_f16x1', *args, wp=wp))    # the |dy| record the _wp call left in amax
  r32 = _dgrad_x2_run(lib, 'conv2d_dgrad_wp_f32', *args, wp=wp)
  torch.cuda.synchronize()
  for r in runs[1:]:
    assert torch.equal(r, runs[0]), 'fp16 twin: launches / prepared weights / records differ in bits'
  assert not torch.equal(runs[0], r32)
  assert amax[512:768].max().item() == dy.abs().max().item()
  sy, sw = _pow2_scale_of(dy.abs().max().item()), _header_scale(blk, wp)
  beta = torch.tensor([0.25] * C1 + [0.75] * C2, dtype=torch.float64)[None, :, None, None]
  acc = beta * dx0.double()
  exact = _dgrad64(_hi(dy, sy), _hi(w, sw), layout, Cin, K, 0.5) + acc
  r64 = _dgrad64(dy, w, layout, Cin, K, 0.5) + acc
  mag = _dgrad64(dy.abs(), w.abs(), layout, Cin, K, 0.5)
  _report(f'dgrad x2 N{N} {C1}+{C2} k{K}', runs[0], exact, r64, mag, scale=(r64 - acc).abs().max().item())


# ---- weight gradient, x and dy as planes: stk_conv2d_wgrad_pl_f16x1 / _wgs_f16x1 ------------------------------------------
WGRAD_PL_CASES = [
  # form, N, Cin, Cout, H, (groups of the default launch, of the 512-workgroup one)
  ('w32', 128, 128, 128, 32),
  ('w16', 128, 256, 256, 16),          # two groups
  ('w8', 128, 256, 256, 8),            # two groups
  ('w4', 128, 256, 256, 4),
  ('w16', 128, 256, 128, 16),          # a short last slab
]


def _wgrad64(x, dy, Cout, K, alpha, pad):
  return torch.nn.grad.conv2d_weight(x.double(), (Cout, x.shape[1], K, K), dy.double(), padding=pad) * alpha


@pytest.mark.parametrize('case', WGRAD_PL_CASES, ids=lambda c: f'{c[0]}_N{c[1]}_{c[2]}to{c[3]}_{c[4]}x{c[4]}')
def test_wgrad_pl_twin(hip_lib, case):
  form, N, Cin, Cout, H = case
  lib = hip_lib
  assert int(lib.conv2d_wgrad_pl_ok(N, H, H, Cin, Cout)) == 1
  nb = int(lib.conv2d_wgrad_pl_ws_bytes(N, H, H, Cin, Cout))
  x = rnd(N, Cin, H, H, seed=41)
  dy = rnd(N, Cout, H, H, seed=42)
  dw0 = rnd(Cout, Cin, 3, 3, seed=43)
  alpha = 0.5
  xd, dyd = x.to(D), dy.to(D)
  rx, ry = _record(lib, xd), _record(lib, dyd)
  xp, yp = _planes(lib, xd, rx), _planes(lib, dyd, ry)
  ws = torch.full((nb // 4 + 64,), float('nan'), device=D)
  out = {}
  for entry, wgs in (('conv2d_wgrad_pl_f16x1', None), ('conv2d_wgrad_pl_wgs_f16x1', 512), ('conv2d_wgrad_pl_f32', None)):
    runs = []
    for _ in range(2):
      dw = dw0.to(D).clone()
      if wgs is None:
        call(lib, entry, xp, rx, yp, ry, dw, alpha, ws, nb, N, H, H, Cin, Cout)
      else:
        call(lib, entry, xp, rx, yp, ry, dw, alpha, ws, nb, N, H, H, Cin, Cout, wgs)
      runs.append(dw.cpu())
    assert torch.equal(runs[0], runs[1]), f'{entry}: two launches differ in bits'
    out[(entry, wgs)] = runs[0]
  assert not torch.equal(out[('conv2d_wgrad_pl_f16x1', None)], out[('conv2d_wgrad_pl_f32', None)])
  sx, sy = _pow2_scale_of(rx.max().item()), _pow2_scale_of(ry.max().item())
  g_exact = _wgrad64(_hi(x, sx), _hi(dy, sy), Cout, 3, alpha, 1)
  g64 = _wgrad64(x, dy, Cout, 3, alpha, 1)
  mag = _wgrad64(x.abs(), dy.abs(), Cout, 3, alpha, 1)
  for (entry, wgs), r in out.items():
    if entry.endswith('_f16x1'):
      _report(f'wgrad pl {form} {Cin}->{Cout} wgs {wgs}', r - dw0, g_exact, g64, mag)


# ---- weight gradient on fp32 operands: stk_conv2d_wgrad_amax_f16x1 (x2::wgemm_kernel with hi-plane loaders) -------------------
WGRAD_X2_CASES = [
  # N, C1, C2, H, Cout, K
  (128, 256, 0, 16, 256, 1),           # 1x1
  (48, 256, 128, 16, 256, 1),          # 1x1 over a concat
  (24, 128, 0, 16, 128, 3),            # 3x3 (the fp32 entry's three-taps kernel; per-tap in the twin)
  (24, 128, 128, 8, 128, 3),           # 3x3 over a concat at 8 x 8
  (128, 256, 0, 4, 256, 3),            # 3x3 on a 4-wide map (per-tap in both)
]


def _wgrad_x2_run(lib, entry, x1d, x2d, C2, dyd, K, dw0d, amax, have):
  N, C1, H, W = x1d.shape
  Cout = dyd.shape[1]
  nb = int(lib.conv2d_wgrad_ws_bytes(C1, C2, N, Cout, H, W, K, K))
  ws = torch.full((nb // 4 + 64,), float('nan'), device=D)
  dw = dw0d.clone()
  call(lib, entry, x1d, C1, x2d, C2, dyd, dw, 0, 0.5, ws, nb, N, H, W, Cout, H, W, K, K, 1, K // 2, amax, have)
  return dw


@pytest.mark.parametrize('case', WGRAD_X2_CASES, ids=lambda c: f'N{c[0]}_{c[1]}+{c[2]}to{c[4]}_{c[3]}x{c[3]}_k{c[5]}')
def test_wgrad_fp32_operand_twin(hip_lib, case):
  N, C1, C2, H, Cout, K = case
  lib = hip_lib
  Cin = C1 + C2
  assert int(lib.conv2d_variant(2, C1, C2, N, H, H, Cout, H, H, K, K, 1, K // 2, 0)) == 5        # the x2 split form
  x1, x2 = rnd(N, C1, H, H, seed=51), (rnd(N, C2, H, H, seed=52, scale=3.0) if C2 else None)
  dy = rnd(N, Cout, H, H, seed=53)
  dw0 = rnd(Cout, Cin, K, K, seed=54)
  x1d, x2d, dyd, dw0d = x1.to(D), (x2.to(D) if C2 else None), dy.to(D), dw0.to(D)
  runs = [_wgrad_x2_run(lib, 'conv2d_wgrad_amax_f16x1', x1d, x2d, C2, dyd, K, dw0d, None, 0) for _ in range(2)]
  # the scale records the forward / data-gradient calls leave behind give the same bits
  amax = torch.zeros(768, device=D)
  call(lib, 'amax_partial_f32', x1d, x1d.numel(), amax)
  if C2:
    call(lib, 'amax_partial_f32', x2d, x2d.numel(), amax[256:])
  call(lib, 'amax_partial_f32', dyd, dyd.numel(), amax[512:])
  runs.append(_wgrad_x2_run(lib, 'conv2d_wgrad_amax_f16x1', x1d, x2d, C2, dyd, K, dw0d, amax, 3))
  r32 = _wgrad_x2_run(lib, 'conv2d_wgrad_amax_f32', x1d, x2d, C2, dyd, K, dw0d, None, 0)
  torch.cuda.synchronize()
  for r in runs[1:]:
    assert torch.equal(r, runs[0]), 'fp16 twin: launches / records differ in bits'
  assert not torch.equal(runs[0], r32)
  x = torch.cat([x1, x2], 1) if C2 else x1
  sx, sy = _pow2_scale_of(x.abs().max().item()), _pow2_scale_of(dy.abs().max().item())
  g_exact = _wgrad64(_hi(x, sx), _hi(dy, sy), Cout, K, 0.5, K // 2)
  g64 = _wgrad64(x, dy, Cout, K, 0.5, K // 2)
  mag = _wgrad64(x.abs(), dy.abs(), Cout, K, 0.5, K // 2)
  _report(f'wgrad x2 N{N} {C1}+{C2}->{Cout} {H}x{H} k{K}', runs[0].cpu() - dw0, g_exact, g64, mag)


# ---- forms without a split: the twin is the fp32 entry ------------------------------------------------------------------
FALLBACK_CASES = [
  # what, N, C, H, Cout, K, stride, OH
  ('thin_in', 16, 3, 64, 128, 3, 1, 64),       # the stem: 3 input channels (weight gradient: thin kernel)
  ('thin_out', 16, 128, 64, 3, 3, 1, 64),      # the head: 3 output channels
  ('t64', 4, 32, 16, 32, 3, 1, 16),            # too few rows / channels for the split kernels
  ('stride2', 16, 128, 32, 128, 3, 2, 16),     # strided downsampling convolution
]


@pytest.mark.parametrize('case', FALLBACK_CASES, ids=[c[0] for c in FALLBACK_CASES])
def test_fallback_forms_are_bitwise_fp32(hip_lib, case):
  what, N, C, H, Cout, K, stride, OH = case
  lib = hip_lib
  assert int(lib.conv2d_variant(1, C, 0, N, H, H, Cout, OH, OH, K, K, stride, 1, 0)) != 5
  assert int(lib.conv2d_variant(2, C, 0, N, H, H, Cout, OH, OH, K, K, stride, 1, 0)) != 5
  x = rnd(N, C, H, H, seed=1).to(D)
  dy = rnd(N, Cout, OH, OH, seed=2).to(D)
  w = _weights(Cout, C, K, 0, seed=3).to(D)
  db = max(int(lib.conv2d_dgrad_ws_bytes(C, 0, N, H, H, Cout, K, K, stride, 1)), 256)
  wb = max(int(lib.conv2d_wgrad_ws_bytes(C, 0, N, Cout, OH, OH, K, K)), 256)
  out = {}
  for sfx in ('_f32', '_f16x1'):
    ws = torch.full((max(db, wb) // 4 + 64,), float('nan'), device=D)
    dx = torch.full((N, C, H, H), float('nan'), device=D)
    amax = torch.zeros(768, device=D)
    call(lib, 'conv2d_dgrad_wp' + sfx, dy, w, 0, dx, C, 0.0, None, 0, 0.0, 1.0, N, H, H, Cout, OH, OH, K, K, stride, 1, None,
         amax, ws, db)
    dw = torch.zeros(Cout, C, K, K, device=D)
    call(lib, 'conv2d_wgrad_amax' + sfx, x, C, None, 0, dy, dw, 0, 1.0, ws, wb, N, H, H, Cout, OH, OH, K, K, stride, 1, None, 0)
    out[sfx] = (dx, dw)
  torch.cuda.synchronize()
  for a, b in zip(out['_f32'], out['_f16x1']):
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
