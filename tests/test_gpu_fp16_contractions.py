"""The one-product forward twins (include/stk_fp16.h; csrc/conv_x2d.h and csrc/conv_x2.h with a OneProduct epilogue) on every
forward launch form.

Each case asserts its launch form through the library's plan diagnostics (as tests/test_gpu_contractions.py does), then:
  - exactness: the result equals the float64 convolution of the fp16 `hi` splits of both operands,
    x~ = fp16_rn(x 2^ex) / 2^ex and w~ = fp16_rn(w 2^ew) / 2^ew, plus the fused epilogue, within fp32 accumulation error.
    The scales are the kernel's own: ex from the |x| scale record the call reads, ew from the |w| maxima in the header of
    the prepared weights (x2::pow2_scale_of: the power of two that puts the bound in [2^13, 2^14)).  This pins "exactly
    one hi * hi product per multiply-add": the three-product fp32 result is 1.3-2.6e-4 of max|y| away from it;
  - against the fp32 inputs: |y - y64| <= (2u + u^2) (|w| * |x|) / out_div + the fp32 term, elementwise, u = 2^-11;
  - repeatability: two launches give identical bits, and so do prepared weights (wp) against weights prepared in ws;
  - the forms that are not split forms (thin-side, f32-input tiles, stride 2) give the fp32 entry's bits exactly.
Errors are printed per case with -s.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import call, rnd
from test_gpu_contractions import _assert_form, _images, _planes, _prepare, _record, _w_oihw, _weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -11
# fp32 accumulation of up to 9 x 256 products and the epilogue, relative to max|y|: measured 1.4-4.0e-7 on these cases
# (MI355X); the fp32 (three-product) result is 1.3-2.6e-4 away from the one-product one
EXACT_RTOL = 2e-6
FP32_TERM = 2e-5           # the fp32 part of the elementwise bound, relative to max|y64|


def _pow2_scale_of(m):
  """x2::pow2_scale_of: 2^(13 - e) for m = 1.f * 2^e (the exponent clamped as in the kernel)"""
  be = int(np.frombuffer(np.float32(m).tobytes(), dtype=np.uint32)[0] >> 23) & 0xff
  if be == 0:
    return 1.0
  se = min(max(127 + 13 - (be - 127), 1), 254)
  return float(2.0 ** (se - 127))


def _hi(t, scale):
  """fp16 `hi` split of an fp32 tensor at a power-of-two scale, back in float64"""
  a = (t.detach().cpu().float().numpy() * np.float32(scale)).astype(np.float16).astype(np.float64) / scale
  return torch.from_numpy(a)


_WPART = 16                # x2::WPART: partial |w| maxima at the front of a prepared-weight block


def _header_scale(blk, ptr):
  """the weight scale the kernels use: x2::weight_scale of the block's header"""
  off = ptr - blk.data_ptr()
  head = blk[off:off + 4 * _WPART].cpu().numpy().view(np.float32)
  return _pow2_scale_of(head.max())


def _ref(xs, w, layout, bias, temb, res, div, K, Cout, idx):
  """float64 forward of the (already split or raw) operands, with the fused epilogue; xs = list of sources"""
  x = torch.cat([t[idx].double() for t in xs], 1)
  out = F.conv2d(x, _w_oihw(w, layout, Cout, x.shape[1], K).double(), padding=K // 2)
  if bias is not None:
    out += bias.double()[None, :, None, None]
  if temb is not None:
    out += temb[idx, 8:8 + Cout].double()[:, :, None, None]
  if res is not None:
    out += res[idx].double()
  return out / float(div)


def _mag(xs, w, layout, K, Cout, idx, div):
  x = torch.cat([t[idx].double().abs() for t in xs], 1)
  return F.conv2d(x, _w_oihw(w, layout, Cout, x.shape[1], K).double().abs(), padding=K // 2) / float(div)


def _checks(label, y, xs_hi, w_hi, xs, w, layout, bias, temb, res, div, K, Cout, N, flops_img):
  idx = _images(N, flops_img)
  got = y.detach().cpu().double()[idx]
  assert torch.isfinite(got).all()
  exact = _ref(xs_hi, w_hi, layout, bias, temb, res, div, K, Cout, idx)
  e_exact = ((got - exact).abs().max() / exact.abs().max()).item()
  y64 = _ref(xs, w, layout, bias, temb, res, div, K, Cout, idx)
  bound = (2 * U + U * U) * _mag(xs, w, layout, K, Cout, idx, div) + FP32_TERM * y64.abs().max()
  excess = ((got - y64).abs() - bound).max().item()
  e_fp32 = ((got - y64).abs().max() / y64.abs().max()).item()
  print(f'  {label}: vs hi*hi float64 {e_exact:.2e} (bound {EXACT_RTOL:.0e}), vs fp32 inputs {e_fp32:.2e}, '
        f'elementwise bound slack {-excess:.3e}')
  assert e_exact <= EXACT_RTOL, f'{label}: not the one-product result: {e_exact:.3e}'
  assert excess <= 0, f'{label}: |y - y64| exceeds (2u + u^2)(|w| * |x|) + fp32 term by {excess:.3e}'


# ---- plane operands: stk_conv2d_fwd_pl_f16x1 ---------------------------------------------------------------------------
PL_CASES = [
  # form, N, C, H, W, Cout, K, layout
  ('h16', 48, 256, 16, 16, 256, 3, 0),
  ('h32', 24, 128, 32, 32, 128, 3, 0),
  ('h32', 24, 96, 32, 32, 128, 3, 0),         # 3 channel groups: the last pair's second slot is the zero DMA
  ('h64', 4, 256, 64, 64, 256, 3, 0),
  ('g9', 4, 128, 128, 128, 128, 3, 0),
  ('g9', 104, 160, 12, 20, 160, 3, 0),        # 20-wide map, 5 channel groups
  ('ks4', 128, 256, 8, 8, 256, 3, 0),
  ('ks3', 128, 160, 8, 8, 256, 3, 0),         # K split over an odd group count
  ('ks6', 128, 256, 4, 4, 256, 3, 0),
  ('g1', 48, 256, 16, 16, 256, 1, 0),         # 1x1 Conv2d layout
  ('g1', 128, 96, 16, 16, 256, 1, 1),         # NIN layout, 3 groups
]


def _pl_id(c):
  return f'{c[0]}_N{c[1]}_{c[2]}to{c[5]}_{c[3]}x{c[4]}_k{c[6]}' + ('_nin' if c[7] else '')


def _pl_run(lib, entry, xd, rec, xp, wd, layout, bd, td, rd, div, K, Cout, wp=None):
  N, C, H, W = xd.shape
  fb = max(int(lib.conv2d_fwd_ws_bytes(C, 0, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=xd.device)
  y = torch.full((N, Cout, H, W), float('nan'), device=xd.device)
  call(lib, entry, xp, rec, C, wd, layout, bd, td.data_ptr() + 4 * 8, td.shape[1], rd, div, y, N, H, W, Cout, K, K, wp, ws, fb)
  return y


@pytest.mark.parametrize('case', PL_CASES, ids=_pl_id)
def test_pl_twin(hip_lib, case):
  form, N, C, H, W, Cout, K, layout = case
  lib = hip_lib
  _assert_form(lib, 0, C, 0, N, H, W, Cout, K, form)
  d = torch.device('cuda:0')
  x = rnd(N, C, H, W, seed=1)
  w = _weights(Cout, C, K, layout, seed=3)
  bias, temb, res = rnd(Cout, seed=4), rnd(N, Cout + 24, seed=5), rnd(N, Cout, H, W, seed=6)
  div = float(np.float32(np.sqrt(2.)))
  xd, wd, bd, td, rd = (t.to(d) for t in (x, w, bias, temb, res))
  rec = _record(lib, xd)
  xp = _planes(lib, xd, rec)
  args = (xd, rec, xp, wd, layout, bd, td, rd, div, K, Cout)
  runs = [_pl_run(lib, 'conv2d_fwd_pl_f16x1', *args) for _ in range(2)]
  blk, wp = _prepare(lib, 0, wd, layout, C, Cout, K, (C, 0, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_pl_run(lib, 'conv2d_fwd_pl_f16x1', *args, wp=wp))
  y32 = _pl_run(lib, 'conv2d_fwd_pl_f32', *args, wp=wp)
  torch.cuda.synchronize()
  for r in runs[1:]:
    assert torch.equal(r, runs[0]), 'fp16 twin: launches / prepared weights differ in bits'
  assert not torch.equal(runs[0], y32), 'the fp16 twin returned the fp32 result'
  sx = _pow2_scale_of(rec.max().item())
  sw = _header_scale(blk, wp)
  assert sw == _pow2_scale_of(w.abs().max().item())
  _checks(f'pl {_pl_id(case)}', runs[0], [_hi(x, sx)], _hi(w, sw), [x], w, layout, bias, temb, res, div, K, Cout, N,
          2.0 * H * W * C * Cout * K * K)


# ---- fp32 operands (the split happens in the loader): stk_conv2d_fwd_wp_f16x1 / _rec_f16x1 ---------------------------------
X2_CASES = [
  # N, C1, C2, H, W, Cout, K, layout
  (128, 256, 0, 16, 16, 256, 1, 1),           # NIN shortcut
  (48, 256, 128, 16, 16, 256, 1, 0),          # the up path's 1x1 shortcut over a concat
  (24, 256, 128, 16, 16, 256, 3, 0),          # a 3x3 over a concat (two sources)
  (128, 256, 256, 4, 4, 256, 3, 0),           # ... small map: K split
]


def _x2_id(c):
  return f'N{c[0]}_{c[1]}+{c[2]}to{c[5]}_{c[3]}x{c[4]}_k{c[6]}' + ('_nin' if c[7] else '')


def _x2_run(lib, entry, x1, x2, C2, wd, layout, bd, td, rd, div, K, Cout, amax, wp=None):
  N, C1, H, W = x1.shape
  fb = max(int(lib.conv2d_fwd_ws_bytes(C1, C2, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=x1.device)
  y = torch.full((N, Cout, H, W), float('nan'), device=x1.device)
  call(lib, entry, x1, C1, x2, C2, wd, layout, bd, td.data_ptr() + 4 * 8, td.shape[1], rd, div, y, N, H, W, Cout, H, W, K, K,
       1, K // 2, wp, amax, ws, fb)
  return y


@pytest.mark.parametrize('case', X2_CASES, ids=_x2_id)
def test_fp32_operand_twin(hip_lib, case):
  N, C1, C2, H, W, Cout, K, layout = case
  lib = hip_lib
  assert int(lib.conv2d_variant(0, C1, C2, N, H, W, Cout, H, W, K, K, 1, K // 2, layout)) == 5     # the x2 split form
  assert C2 > 0 or int(lib.conv2d_pl_ok(0, C1, 0, N, H, W, Cout, K, K, 1, K // 2)) == 1
  d = torch.device('cuda:0')
  x1, x2 = rnd(N, C1, H, W, seed=1), (rnd(N, C2, H, W, seed=2, scale=3.0) if C2 else None)
  w = _weights(Cout, C1 + C2, K, layout, seed=3)
  bias, temb, res = rnd(Cout, seed=4), rnd(N, Cout + 24, seed=5), rnd(N, Cout, H, W, seed=6)
  div = float(np.float32(np.sqrt(2.)))
  x1d, wd, bd, td, rd = (t.to(d) for t in (x1, w, bias, temb, res))
  x2d = x2.to(d) if C2 else None
  amax = torch.zeros(768, device=d)
  args = (x1d, x2d, C2, wd, layout, bd, td, rd, div, K, Cout, amax)
  runs = [_x2_run(lib, 'conv2d_fwd_wp_f16x1', *args) for _ in range(2)]
  blk, wp = _prepare(lib, 0, wd, layout, C1 + C2, Cout, K, (C1, C2, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_x2_run(lib, 'conv2d_fwd_wp_f16x1', *args, wp=wp))
  runs.append(_x2_run(lib, 'conv2d_fwd_rec_f16x1', *args, wp=wp))      # the records the _wp call left in amax
  y32 = _x2_run(lib, 'conv2d_fwd_wp_f32', *args, wp=wp)
  torch.cuda.synchronize()
  for r in runs[1:]:
    assert torch.equal(r, runs[0]), 'fp16 twin: launches / prepared weights / records differ in bits'
  assert not torch.equal(runs[0], y32)
  m = max(x1.abs().max().item(), x2.abs().max().item() if C2 else 0.0)
  assert amax[:512 if C2 else 256].max().item() == m
  sx, sw = _pow2_scale_of(m), _header_scale(blk, wp)
  xs = [x1] + ([x2] if C2 else [])
  _checks(f'x2 {_x2_id(case)}', runs[0], [_hi(t, sx) for t in xs], _hi(w, sw), xs, w, layout, bias, temb, res, div, K, Cout,
          N, 2.0 * H * W * (C1 + C2) * Cout * K * K)


# ---- forms without a split: the twin is the fp32 entry ------------------------------------------------------------------
FALLBACK_CASES = [
  # what, N, C1, H, W, Cout, K, stride, OH, OW, variant
  ('thin_in', 16, 3, 64, 64, 128, 3, 1, 64, 64, 4),       # the stem: 3 input channels
  ('thin_out', 16, 128, 64, 64, 3, 3, 1, 64, 64, 4),      # the head: 3 output channels
  ('t64', 4, 64, 16, 16, 64, 3, 1, 16, 16, 0),           # too few rows for the split kernels
  ('stride2', 16, 128, 32, 32, 128, 3, 2, 16, 16, 0),     # strided downsampling convolution
]


@pytest.mark.parametrize('case', FALLBACK_CASES, ids=[c[0] for c in FALLBACK_CASES])
def test_fallback_forms_are_bitwise_fp32(hip_lib, case):
  what, N, C, H, W, Cout, K, stride, OH, OW, variant = case
  lib = hip_lib
  assert int(lib.conv2d_variant(0, C, 0, N, H, W, Cout, OH, OW, K, K, stride, 1, 0)) == variant
  d = torch.device('cuda:0')
  x = rnd(N, C, H, W, seed=1).to(d)
  w = _weights(Cout, C, K, 0, seed=3).to(d)
  bias = rnd(Cout, seed=4).to(d)
  fb = max(int(lib.conv2d_fwd_ws_bytes(C, 0, N, H, W, Cout, K, K, stride, 1)), 256)
  out = {}
  for entry in ('conv2d_fwd_wp_f32', 'conv2d_fwd_wp_f16x1'):
    ws = torch.full((fb // 4 + 64,), float('nan'), device=d)
    y = torch.full((N, Cout, OH, OW), float('nan'), device=d)
    amax = torch.zeros(768, device=d)
    call(lib, entry, x, C, None, 0, w, 0, bias, None, 0, None, 1.0, y, N, H, W, Cout, OH, OW, K, K, stride, 1, None, amax, ws,
         fb)
    out[entry] = y
  torch.cuda.synchronize()
  assert torch.isfinite(out['conv2d_fwd_wp_f32']).all()
  assert torch.equal(out['conv2d_fwd_wp_f16x1'], out['conv2d_fwd_wp_f32'])
