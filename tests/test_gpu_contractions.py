"""The plane-operand contractions (csrc/conv_x2d.h, csrc/conv_x2w.h) against float64, on every launch form.

Each case first asserts the form it is meant to reach, through the library's own plan diagnostics (stk_conv2d_pl_halo,
stk_conv2d_pl_ksplit, stk_conv2d_pl_ok, stk_conv2d_wgrad_pl_ok, stk_conv2d_wgrad_pl_ws_bytes), so a planner change cannot
move a case off its kernel unnoticed.  The oracle does not restate the planner, so those assertions only run on the
device.  The reference is torch in float64 on the fp32 inputs -- not the oracle and not the decoded planes -- so an error
in the split itself shows too.  Every launch runs twice and must repeat bit for bit (LDS-DMA pipelines, fixed slab
order); forward and data-gradient cases run once more on weights prepared by stk_conv2d_wprep_batch, which must give the
same bits.  Errors are max|got - ref| / max|ref|, printed per case with -s, bounded by tests/_tolerances.py.

Launch forms (csrc/conv.hip split_plan / launch_split / split_gemm, x2w::plan):
  h16 / h32 / h64   x2d::gemm_halo_kernel<W>: 3x3, >= 192 tiles of 128 x 128 (no K split), W in {16, 32, 64}
  g9 / g1           x2d::gemm_kernel<9 | 1>: un-split, other widths / 1x1 (Conv2d and NIN layouts)
  ks                the K-split EpSlab form + the slab sum (< 192 tiles)
  w32 / w16 / w8 / w4   x2w::wgrad_kernel<COLS> (one group on the 32- and 4-wide maps, two on the 16- and 8-wide ones)
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _tolerances import PL_DGRAD_RTOL, PL_FWD_RTOL, PL_WGRAD_RTOL
import _gn_cases as gc
from _util import call, dev_of, rnd

pytestmark = pytest.mark.gpu

# with the oracle standing in (STK_SELFCHECK, CPU) only the cases its plain-C loops finish in seconds run
_SELFCHECK_FLOPS = 8e9
# host float64 reference: at most this many multiply-adds per case (images are independent in fwd / dgrad: a spread subset)
_REF_FLOPS = 1.2e10


class _WprepDesc(ctypes.Structure):       # StkWprepDesc of include/stk.h
  _fields_ = [('w', ctypes.c_void_p), ('wp', ctypes.c_void_p), ('sm', ctypes.c_long), ('sk', ctypes.c_long),
              ('M', ctypes.c_int), ('Kc', ctypes.c_int), ('Mpad', ctypes.c_int), ('taps', ctypes.c_int),
              ('flip', ctypes.c_int), ('reserved', ctypes.c_int)]


class _GnFoldDesc(ctypes.Structure):      # StkGnFoldDesc of include/stk.h
  _fields_ = [('part', ctypes.c_void_p), ('dgamma', ctypes.c_void_p), ('dbeta', ctypes.c_void_p),
              ('N', ctypes.c_int), ('C', ctypes.c_int)]


def _table(structs, d):
  raw = b''.join(bytes(s) for s in structs)
  return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(d)


def _size_gate(lib, flops):
  if not lib.is_device and flops > _SELFCHECK_FLOPS:
    pytest.skip('the plain-C checker is too slow for this size (runs on the device)')


def _sync(lib):
  if lib.is_device:
    torch.cuda.synchronize()


def _images(N, flops_per_image):
  """indices of the images the host reference covers: all of them, or a spread subset with both ends."""
  k = int(max(2, min(N, _REF_FLOPS // max(flops_per_image, 1))))
  return sorted(set(np.linspace(0, N - 1, k).round().astype(int).tolist()))


def _err(got, ref):
  got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
  assert got.shape == ref.shape, (got.shape, ref.shape)
  assert torch.isfinite(got).all(), 'non-finite result'
  return ((got - ref).abs().max() / ref.abs().max()).item()


def _check(label, errs, bound):
  print(f'  {label}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()) + f'  (bound {bound:.0e})')
  for k, v in errs.items():
    assert v <= bound, f'{label} {k}: max|err| / max|ref| = {v:.3e} > {bound:.0e}'


def _same(runs, what):
  """every launch of the list must have produced the same bits"""
  for i, r in enumerate(runs[1:], 1):
    for k in r:
      assert torch.equal(r[k], runs[0][k]), f'{what}: {k} of run {i} differs from run 0'


def _record(lib, t):
  rec = torch.zeros(256, device=t.device)
  call(lib, 'amax_partial_f32', t, t.numel(), rec)
  return rec


def _planes(lib, t, rec):
  N, C = t.shape[:2]
  HW = t[0, 0].numel()
  pl = torch.zeros(int(lib.planes_bytes(N, C, HW)), dtype=torch.uint8, device=t.device)
  call(lib, 'split_planes_f32', t, N, C, HW, rec, 256, pl)
  return pl


def _prepare(lib, direction, w, layout, Cin, Cout, K, shape):
  """the layer's prepared-weight block of one direction, as the engine makes it (one stk_conv2d_wprep_batch launch)"""
  if not lib.is_device:
    return None, None          # the checker has no prepared weights (its _wp / _pl entries ignore wp)
  nb = int(lib.conv2d_wp_bytes(direction, *shape))
  assert nb > 0, ('no prepared-weight block', direction, shape)
  blk = torch.full((nb + 256,), 0xff, dtype=torch.uint8, device=w.device)
  ptr = (blk.data_ptr() + 255) // 256 * 256
  desc = _WprepDesc()
  n = lib.conv2d_wp_desc(direction, w.data_ptr(), layout, Cin, Cout, K, K, ptr, ctypes.byref(desc))
  assert n > 0
  call(lib, 'conv2d_wprep_batch', _table([desc], w.device), 1, n)
  return blk, ptr


def _assert_form(lib, direction, C1, C2, N, H, W, Cout, K, form):
  """the planner takes this call to the kernel named by `form` (device only: the oracle does not restate the plan)"""
  assert int(lib.conv2d_pl_ok(direction, C1, C2, N, H, W, Cout, K, K, 1, K // 2)) == 1
  if not lib.is_device:
    return
  ks = int(lib.conv2d_pl_ksplit(direction, C1, C2, N, H, W, Cout, K, K))
  halo = int(lib.conv2d_pl_halo(direction, C1, C2, N, H, W, Cout, K, K))
  got = (f'h{halo}' if halo else ('g9' if K == 3 else 'g1')) if ks == 1 else f'ks{ks}'
  assert got == form, (form, got, (direction, C1, C2, N, H, W, Cout, K))


def _weights(Cout, Cin, K, layout, seed):
  if layout == 1:
    return rnd(Cin, Cout, seed=seed) / np.sqrt(Cin)
  return rnd(Cout, Cin, K, K, seed=seed) / np.sqrt(Cin * K * K)


def _w_oihw(w, layout, Cout, Cin, K):
  return w.t().reshape(Cout, Cin, 1, 1) if layout == 1 else w


# ---- forward ----------------------------------------------------------------------------------------------------------
FWD_CASES = [
  # form, N, C, H, W, Cout, K, layout
  ('h16', 48, 256, 16, 16, 256, 3, 0),
  ('h16', 128, 256, 16, 16, 256, 3, 0),      # BASELINE: DDPM++ 16 x 16 level, batch 128
  ('h32', 24, 128, 32, 32, 128, 3, 0),
  ('h32', 128, 128, 32, 32, 128, 3, 0),      # BASELINE: DDPM++ 32 x 32 level, batch 128
  ('h64', 6, 128, 64, 64, 128, 3, 0),
  ('h64', 4, 256, 64, 64, 256, 3, 0),        # BASELINE: NCSN++ 256^2 net, 64 x 64 level, batch 4
  ('g9', 4, 128, 128, 128, 128, 3, 0),       # BASELINE: NCSN++ 256^2 net, 128 x 128 level, batch 4
  ('g9', 4, 128, 256, 256, 128, 3, 0),       # ... 256 x 256 level
  ('g9', 104, 128, 12, 20, 160, 3, 0),       # a 20-wide map: ragged pixel tiles across images, 160 rows
  ('ks4', 128, 256, 8, 8, 256, 3, 0),        # BASELINE: 8 x 8 level, batch 128
  ('ks6', 128, 256, 4, 4, 256, 3, 0),        # BASELINE: 4 x 4 level, batch 128
  ('ks6', 4, 256, 32, 32, 256, 3, 0),        # 32 x 32 at batch 4
  ('g1', 48, 256, 16, 16, 256, 1, 0),        # 1x1 Conv2d
  ('g1', 128, 256, 16, 16, 256, 1, 1),       # BASELINE: the attention block's NIN at 16 x 16, batch 128
]


def _fwd_id(c):
  return f'{c[0]}_N{c[1]}_{c[2]}to{c[5]}_{c[3]}x{c[4]}_k{c[6]}' + ('_nin' if c[7] else '')


def _fwd_run(lib, x, w, layout, bias, temb, res, div, K, Cout, wp=None):
  N, C, H, W = x.shape
  d = x.device
  fb = max(int(lib.conv2d_fwd_ws_bytes(C, 0, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=d)
  rec = _record(lib, x)
  xp = _planes(lib, x, rec)
  y = torch.full((N, Cout, H, W), float('nan'), device=d)
  tptr, tstride = (temb.data_ptr() + 4 * 8, temb.shape[1]) if temb is not None else (None, 0)
  call(lib, 'conv2d_fwd_pl_f32', xp, rec, C, w, layout, bias, tptr, tstride, res, div, y, N, H, W, Cout, K, K, wp, ws, fb)
  return y


def _fwd_ref(x, w, layout, bias, temb, res, div, K, Cout, idx):
  C = x.shape[1]
  ref = F.conv2d(x[idx].double(), _w_oihw(w, layout, Cout, C, K).double(), padding=K // 2)
  if bias is not None:
    ref += bias.double()[None, :, None, None]
  if temb is not None:
    ref += temb[idx, 8:8 + Cout].double()[:, :, None, None]
  if res is not None:
    ref += res[idx].double()
  return ref / float(div)


@pytest.mark.parametrize('case', FWD_CASES, ids=_fwd_id)
def test_forward_from_planes(hip_lib, case):
  form, N, C, H, W, Cout, K, layout = case
  lib = hip_lib
  _size_gate(lib, 2.0 * N * H * W * C * Cout * K * K)
  _assert_form(lib, 0, C, 0, N, H, W, Cout, K, form)
  d = dev_of(lib)
  x = rnd(N, C, H, W, seed=1)
  w = _weights(Cout, C, K, layout, seed=3)
  bias = rnd(Cout, seed=4)
  temb = rnd(N, Cout + 24, seed=5)            # read as the column slice [8, 8 + Cout) of a wider tensor
  res = rnd(N, Cout, H, W, seed=6)
  div = float(np.float32(np.sqrt(2.)))
  xd, wd, bd, td, rd = (t.to(d) for t in (x, w, bias, temb, res))
  runs = [_fwd_run(lib, xd, wd, layout, bd, td, rd, div, K, Cout) for _ in range(2)]
  blk, wp = _prepare(lib, 0, wd, layout, C, Cout, K, (C, 0, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_fwd_run(lib, xd, wd, layout, bd, td, rd, div, K, Cout, wp=wp))
  _sync(lib)
  _same([{'y': r} for r in runs], 'forward (wp = NULL twice, prepared weights)')
  idx = _images(N, 2.0 * H * W * C * Cout * K * K)
  ref = _fwd_ref(x, w, layout, bias, temb, res, div, K, Cout, idx)
  _check(f'fwd {form} {_fwd_id(case)}', {'y': _err(runs[0].cpu()[idx], ref)}, PL_FWD_RTOL)


# ---- data gradient ----------------------------------------------------------------------------------------------------
DGRAD_CASES = [
  # form, N, C1, C2, H, W, Cout, K, layout
  ('h16', 24, 256, 256, 16, 16, 256, 3, 0),   # up path at 16 x 16: 256 + 256 -> 256
  ('h16', 48, 160, 96, 16, 16, 256, 3, 0),    # the C1 boundary inside a 128-row tile
  ('h16', 128, 256, 0, 16, 16, 256, 3, 0),    # BASELINE, batch 128
  ('h32', 8, 256, 128, 32, 32, 128, 3, 0),    # up path at 32 x 32: 256 + 128 -> 128
  ('h32', 12, 96, 160, 32, 32, 128, 3, 0),    # C1 boundary inside the first row tile
  ('h32', 128, 128, 0, 32, 32, 128, 3, 0),    # BASELINE, batch 128
  ('h64', 3, 128, 128, 64, 64, 128, 3, 0),
  ('h64', 3, 160, 96, 64, 64, 128, 3, 0),
  ('h64', 4, 256, 0, 64, 64, 256, 3, 0),      # BASELINE: 256^2 net at batch 4
  ('g9', 4, 128, 0, 128, 128, 128, 3, 0),     # BASELINE: 256^2 net at batch 4, 128 x 128
  ('g9', 4, 128, 128, 128, 128, 128, 3, 0),   # ... its up-path concat
  ('g9', 4, 128, 0, 256, 256, 128, 3, 0),     # ... 256 x 256
  ('g9', 104, 128, 0, 12, 20, 160, 3, 0),     # 20-wide map, ragged pixel tiles
  ('ks4', 128, 256, 0, 8, 8, 256, 3, 0),      # BASELINE 8 x 8
  ('ks6', 128, 256, 0, 4, 4, 256, 3, 0),      # BASELINE 4 x 4
  ('ks6', 4, 256, 0, 32, 32, 256, 3, 0),      # 32 x 32 at batch 4
  ('g9', 128, 256, 256, 8, 8, 256, 3, 0),     # BASELINE up path at 8 x 8 (512 rows: enough tiles), two sources
  ('g1', 48, 256, 0, 16, 16, 256, 1, 0),      # 1x1 Conv2d
  ('g1', 128, 256, 0, 16, 16, 256, 1, 1),     # BASELINE NIN
]


def _dgrad_id(c):
  return f'{c[0]}_N{c[1]}_{c[2]}+{c[3]}from{c[6]}_{c[4]}x{c[5]}_k{c[7]}' + ('_nin' if c[8] else '')


def _dgrad_run(lib, dy, w, layout, C1, C2, K, dx1_0, dx2_0, beta1, beta2, alpha, wp=None):
  N, Cout, H, W = dy.shape
  d = dy.device
  fb = max(int(lib.conv2d_dgrad_ws_bytes(C1, C2, N, H, W, Cout, K, K, 1, K // 2)), 256)
  ws = torch.full((fb // 4 + 64,), float('nan'), device=d)
  rec = _record(lib, dy)
  yp = _planes(lib, dy, rec)
  # beta == 0: dx is overwritten, never read -- it starts as NaN
  dx1 = dx1_0.clone() if beta1 else torch.full((N, C1, H, W), float('nan'), device=d)
  dx2 = (dx2_0.clone() if beta2 else torch.full((N, C2, H, W), float('nan'), device=d)) if C2 else None
  call(lib, 'conv2d_dgrad_pl_f32', yp, rec, w, layout, dx1, C1, beta1, dx2, C2, beta2, alpha, N, H, W, Cout, K, K, wp, ws,
       fb)
  return {'dx1': dx1, 'dx2': dx2} if C2 else {'dx1': dx1}


def _dgrad_ref(dy, w, layout, C1, C2, K, dx1_0, dx2_0, beta1, beta2, alpha, idx):
  Cout, H, W = dy.shape[1:]
  full = torch.nn.grad.conv2d_input((len(idx), C1 + C2, H, W), _w_oihw(w, layout, Cout, C1 + C2, K).double(),
                                    dy[idx].double(), padding=K // 2) * alpha
  out = {'dx1': full[:, :C1] + beta1 * dx1_0[idx].double()}
  if C2:
    out['dx2'] = full[:, C1:] + beta2 * dx2_0[idx].double()
  return out


@pytest.mark.parametrize('case', DGRAD_CASES, ids=_dgrad_id)
def test_data_gradient_from_planes(hip_lib, case):
  """dx1 overwritten (two sources) or accumulated (one), dx2 accumulated, alpha != 1: the row routing of a concat input."""
  form, N, C1, C2, H, W, Cout, K, layout = case
  lib = hip_lib
  Cin = C1 + C2
  _size_gate(lib, 2.0 * N * H * W * Cin * Cout * K * K)
  _assert_form(lib, 1, C1, C2, N, H, W, Cout, K, form)
  d = dev_of(lib)
  dy = rnd(N, Cout, H, W, seed=7)
  w = _weights(Cout, Cin, K, layout, seed=3)
  dx1_0, dx2_0 = rnd(N, C1, H, W, seed=8), (rnd(N, C2, H, W, seed=9) if C2 else None)
  beta1, beta2, alpha = (0.0, 0.75, 0.5) if C2 else (0.25, 0.0, 0.5)
  dyd, wd = dy.to(d), w.to(d)
  a1, a2 = dx1_0.to(d), (dx2_0.to(d) if C2 else None)
  args = (layout, C1, C2, K, a1, a2, beta1, beta2, alpha)
  runs = [_dgrad_run(lib, dyd, wd, *args) for _ in range(2)]
  blk, wp = _prepare(lib, 1, wd, layout, Cin, Cout, K, (C1, C2, N, H, W, Cout, K, K, 1, K // 2))
  runs.append(_dgrad_run(lib, dyd, wd, *args, wp=wp))
  _sync(lib)
  _same(runs, 'data gradient (wp = NULL twice, prepared weights)')
  idx = _images(N, 2.0 * H * W * Cin * Cout * K * K)
  ref = _dgrad_ref(dy, w, layout, C1, C2, K, dx1_0, dx2_0, beta1, beta2, alpha, idx)
  _check(f'dgrad {form} {_dgrad_id(case)}', {k: _err(runs[0][k].cpu()[idx], ref[k]) for k in ref}, PL_DGRAD_RTOL)


# ---- realistic operands -----------------------------------------------------------------------------------------------
SPREAD_CASES = [
  # form, N, C, H, W, Cout
  ('h32', 24, 128, 32, 32, 128),
  ('h16', 48, 256, 16, 16, 256),
  ('g9', 104, 128, 12, 20, 160),
  ('ks4', 128, 256, 8, 8, 256),
  ('ks6', 4, 256, 32, 32, 256),
]


def _spread(N, seed):
  """per-image factors over 4 decades in a shuffled order, as the loss weights of a batch of noise levels make them"""
  g = torch.Generator().manual_seed(seed)
  return torch.logspace(-4, 0, N)[torch.randperm(N, generator=g)][:, None, None, None]


@pytest.mark.parametrize('case', SPREAD_CASES, ids=lambda c: f'{c[0]}_N{c[1]}_{c[2]}to{c[5]}_{c[3]}x{c[4]}')
def test_spread_operand_per_image(hip_lib, case):
  """The activation / gradient operand with per-image magnitudes over 4 decades: one scale serves the whole batch, so the
  small images live in the low bits of the planes.  Each image must still be right relative to its own magnitude."""
  form, N, C, H, W, Cout = case
  lib = hip_lib
  _size_gate(lib, 4.0 * N * H * W * C * Cout * 9)
  _assert_form(lib, 0, C, 0, N, H, W, Cout, 3, form)
  _assert_form(lib, 1, C, 0, N, H, W, Cout, 3, form)
  d = dev_of(lib)
  x = rnd(N, C, H, W, seed=11) * _spread(N, 1)
  dy = rnd(N, Cout, H, W, seed=12) * _spread(N, 2)
  w = _weights(Cout, C, 3, 0, seed=13)
  xd, dyd, wd = x.to(d), dy.to(d), w.to(d)
  ys = [_fwd_run(lib, xd, wd, 0, None, None, None, 1.0, 3, Cout) for _ in range(2)]
  dxs = [_dgrad_run(lib, dyd, wd, 0, C, 0, 3, None, None, 0.0, 0.0, 1.0) for _ in range(2)]
  _sync(lib)
  _same([{'y': y} for y in ys], 'forward')
  _same(dxs, 'data gradient')
  idx = _images(N, 4.0 * H * W * C * Cout * 9)
  yr = F.conv2d(x[idx].double(), w.double(), padding=1)
  dxr = torch.nn.grad.conv2d_input((len(idx), C, H, W), w.double(), dy[idx].double(), padding=1)
  y, dx = ys[0].cpu()[idx], dxs[0]['dx1'].cpu()[idx]
  errs = {'y': _err(y, yr), 'dx': _err(dx, dxr),
          'y per image': max(_err(y[i], yr[i]) for i in range(len(idx))),
          'dx per image': max(_err(dx[i], dxr[i]) for i in range(len(idx)))}
  _check(f'spread {form}', {k: v for k, v in errs.items() if k.startswith('y')}, PL_FWD_RTOL)
  _check(f'spread {form}', {k: v for k, v in errs.items() if k.startswith('dx')}, PL_DGRAD_RTOL)


@pytest.mark.parametrize('case', [('h32', 24, 128, 32, 32, 128), ('ks4', 128, 256, 8, 8, 256), ('g1', 48, 256, 16, 16, 256)],
                         ids=lambda c: f'{c[0]}_N{c[1]}')
def test_power_of_two_maximum(hip_lib, case):
  """|max| of the operand exactly a power of two: the floor(log2) edge of the planes' scale (the maximum maps to 2^13)."""
  form, N, C, H, W, Cout = case
  K = 1 if form == 'g1' else 3
  lib = hip_lib
  _size_gate(lib, 4.0 * N * H * W * C * Cout * K * K)
  _assert_form(lib, 0, C, 0, N, H, W, Cout, K, form)
  _assert_form(lib, 1, C, 0, N, H, W, Cout, K, form)
  d = dev_of(lib)
  x = rnd(N, C, H, W, seed=21).clamp(-3.9, 3.9)
  x[N - 1, C // 2, H // 2, W - 1] = -4.0
  dy = rnd(N, Cout, H, W, seed=22).clamp(-0.49, 0.49)
  dy[0, 0, 0, 0] = 0.5
  w = _weights(Cout, C, K, 0, seed=23)
  xd, dyd, wd = x.to(d), dy.to(d), w.to(d)
  y = _fwd_run(lib, xd, wd, 0, None, None, None, 1.0, K, Cout)
  dx = _dgrad_run(lib, dyd, wd, 0, C, 0, K, None, None, 0.0, 0.0, 1.0)['dx1']
  _sync(lib)
  idx = _images(N, 4.0 * H * W * C * Cout * K * K)
  yr = F.conv2d(x[idx].double(), w.double(), padding=K // 2)
  dxr = torch.nn.grad.conv2d_input((len(idx), C, H, W), w.double(), dy[idx].double(), padding=K // 2)
  _check(f'pow2 max {form}', {'y': _err(y.cpu()[idx], yr)}, PL_FWD_RTOL)
  _check(f'pow2 max {form}', {'dx': _err(dx.cpu()[idx], dxr)}, PL_DGRAD_RTOL)


@pytest.mark.parametrize('case', [('h32', 24, 128, 32, 32, 128), ('ks4', 128, 256, 8, 8, 256), ('g1', 48, 256, 16, 16, 256)],
                         ids=lambda c: f'{c[0]}_N{c[1]}')
def test_all_zero_operand(hip_lib, case):
  """An all-zero operand (record maximum 0: scale 1, planes all zero): the forward is the epilogue terms alone, the data
  gradient leaves beta dx, the weight gradient leaves dw -- to fp32 rounding, and nowhere a NaN."""
  form, N, C, H, W, Cout = case
  K = 1 if form == 'g1' else 3
  lib = hip_lib
  _size_gate(lib, 2.0 * N * H * W * C * Cout * K * K)
  _assert_form(lib, 0, C, 0, N, H, W, Cout, K, form)
  _assert_form(lib, 1, C, 0, N, H, W, Cout, K, form)
  d = dev_of(lib)
  w = _weights(Cout, C, K, 0, seed=31)
  bias, temb, res = rnd(Cout, seed=32), rnd(N, Cout + 24, seed=33), rnd(N, Cout, H, W, seed=34)
  div = float(np.float32(np.sqrt(2.)))
  x0, dy0 = torch.zeros(N, C, H, W, device=d), torch.zeros(N, Cout, H, W, device=d)
  dx_0 = rnd(N, C, H, W, seed=35)
  y = _fwd_run(lib, x0, w.to(d), 0, bias.to(d), temb.to(d), res.to(d), div, K, Cout)
  dx = _dgrad_run(lib, dy0, w.to(d), 0, C, 0, K, dx_0.to(d), None, 0.75, 0.0, 0.5)['dx1']
  out = {'y': y.cpu(), 'dx': dx.cpu()}
  if K == 3 and int(lib.conv2d_wgrad_pl_ok(N, H, W, C, Cout)):
    nb = int(lib.conv2d_wgrad_pl_ws_bytes(N, H, W, C, Cout))
    ws = torch.full((nb // 4 + 64,), float('nan'), device=d)
    rx, ry = _record(lib, x0), _record(lib, dy0)
    dw = rnd(Cout, C, 3, 3, seed=36).to(d)
    dw_0 = dw.clone()
    call(lib, 'conv2d_wgrad_pl_f32', _planes(lib, x0, rx), rx, _planes(lib, dy0, ry), ry, dw, 0.5, ws, nb, N, H, W, C, Cout)
    out['dw'] = dw.cpu()
    assert torch.equal(out['dw'], dw_0.cpu())
  _sync(lib)
  for k, v in out.items():
    assert not torch.isnan(v).any(), k
  yr = (bias.double()[None, :, None, None] + temb[:, 8:8 + Cout].double()[:, :, None, None] + res.double()) / div
  _check(f'zero operand {form}', {'y': _err(out['y'], yr), 'dx': _err(out['dx'], 0.75 * dx_0.double())}, 1e-6)


# ---- weight gradient --------------------------------------------------------------------------------------------------
WGRAD_CASES = [
  # form, N, Cin, Cout, H, slabs (stk_conv2d_wgrad_pl_ws_bytes: the deepest K split any workgroup count asks for)
  ('w32', 128, 128, 128, 32, 216),     # BASELINE: DDPM++ 32 x 32, batch 128 (one group)
  ('w16', 128, 256, 256, 16, 28),      # 16 x 16 (two groups)
  ('w8', 128, 256, 256, 8, 16),        # 8 x 8 (two groups)
  ('w4', 128, 256, 256, 4, 8),         # 4 x 4 (one group)
  ('w16', 128, 256, 128, 16, 103),     # the 256 -> 128 layer at 16 x 16: a short last slab
]


@pytest.mark.parametrize('case', WGRAD_CASES, ids=lambda c: f'{c[0]}_N{c[1]}_{c[2]}to{c[3]}_{c[4]}x{c[4]}')
def test_weight_gradient_from_planes(hip_lib, case):
  """dw += alpha sum dy x with both operands as planes, through the default launch (256 workgroups) and with 512, each
  twice; dy spread over 4 decades per image.  The error is relative to max|alpha sum dy x|, not to the accumulated dw."""
  _weight_gradient_from_planes(hip_lib, case, tiny=False)


def test_weight_gradient_from_planes_tiny_operands(hip_lib):
  """The same with max|x| = 2^-60 and max|dy| = 2^-50 into a zero dw: the two scales multiply to 2^136, past fp32, and the
  gradient (about 2^-105) is a normal fp32 number.  `unscale` formed as 1 / (sa sb) is 0 there and dw stays 0."""
  _weight_gradient_from_planes(hip_lib, ('w8', 128, 256, 256, 8, 16), tiny=True)


def _weight_gradient_from_planes(lib, case, tiny):
  form, N, Cin, Cout, H, slabs = case
  _size_gate(lib, 2.0 * N * H * H * Cin * Cout * 9)
  assert int(lib.conv2d_wgrad_pl_ok(N, H, H, Cin, Cout)) == 1
  nb = int(lib.conv2d_wgrad_pl_ws_bytes(N, H, H, Cin, Cout))
  if lib.is_device:
    assert nb == slabs * 9 * Cin * Cout * 4 + 256, (nb, slabs)
  d = dev_of(lib)
  x = rnd(N, Cin, H, H, seed=41)
  dy = rnd(N, Cout, H, H, seed=42) * _spread(N, 3)
  dw0 = rnd(Cout, Cin, 3, 3, seed=43)
  if tiny:
    x, dy = x / x.abs().max() * 2.0 ** -60, dy / dy.abs().max() * 2.0 ** -50
    dw0 = torch.zeros_like(dw0)
  alpha = 0.5
  xd, dyd = x.to(d), dy.to(d)
  rx, ry = _record(lib, xd), _record(lib, dyd)
  xp, yp = _planes(lib, xd, rx), _planes(lib, dyd, ry)
  ws = torch.full((nb // 4 + 64,), float('nan'), device=d)
  runs = {}
  for name, wgs in (('default', None), ('wgs512', 512)):
    outs = []
    for _ in range(2):
      dw = dw0.to(d).clone()
      if wgs is None:
        call(lib, 'conv2d_wgrad_pl_f32', xp, rx, yp, ry, dw, alpha, ws, nb, N, H, H, Cin, Cout)
      else:
        call(lib, 'conv2d_wgrad_pl_wgs_f32', xp, rx, yp, ry, dw, alpha, ws, nb, N, H, H, Cin, Cout, wgs)
      outs.append({'dw': dw.cpu()})
    _same(outs, f'weight gradient ({name})')
    runs[name] = outs[0]['dw']
  _sync(lib)
  g = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dy.double(), padding=1) * alpha
  ref = dw0.double() + g
  scale = g.abs().max().item()
  errs = {k: (v.double() - ref).abs().max().item() / scale for k, v in runs.items()}
  _check(f'wgrad {form} N{N} {Cin}->{Cout} {H}x{H}', errs, PL_WGRAD_RTOL)


# ---- the step's entry points around the contractions ------------------------------------------------------------------
@pytest.mark.parametrize('case', [(8, 256, 256), (5, 128, 64), (128, 256, 16)], ids=str)
def test_bias_grad_amax_dual(ref_lib, hip_lib, case):
  """stk_bias_grad_amax_dual_f32: dbias += and dbias2 += the same sums, dtemb written, both scale records' maxima ==
  max|dy| exactly (a maximum has no rounding)."""
  N, C, HW = case
  dy = rnd(N, C, HW, seed=51) * torch.logspace(-3, 1, N)[:, None, None]
  out = {}
  for name, lib in (('ref', ref_lib), ('hip', hip_lib)):
    d = dev_of(lib)
    db, db2 = rnd(C, seed=52).to(d), rnd(C, seed=53).to(d)
    dt = torch.full((N, C + 8), float('nan'), device=d)
    rec, rec2 = torch.full((256,), float('nan'), device=d), torch.full((256,), float('nan'), device=d)
    ws = torch.zeros(N * C + 64, device=d)
    call(lib, 'bias_grad_amax_dual_f32', dy.to(d), N, C, HW, 0.5, dt, C + 8, db, rec, db2, rec2, ws)
    out[name] = dict(db=db.cpu(), db2=db2.cpu(), dt=dt.cpu()[:, :C], rec=rec.cpu(), rec2=rec2.cpu())
  r, h = out['ref'], out['hip']
  m = float(dy.abs().max())
  for k in ('rec', 'rec2'):
    assert float(h[k].max()) == m, k
    assert not torch.isnan(h[k]).any() and float(h[k].min()) >= 0, k
  s = 0.5 * dy.double().sum(2)
  for k, want in (('db', rnd(C, seed=52).double() + s.sum(0)), ('db2', rnd(C, seed=53).double() + s.sum(0)), ('dt', s)):
    assert (h[k].double() - want).abs().max().item() <= 1e-5 * want.abs().max().item(), k
    assert (h[k] - r[k]).abs().max().item() <= 1e-5 * r[k].abs().max().item(), k


@pytest.mark.parametrize('case', [(128, 256, 16, 256, 256), (128, 256, 8, 256, 256), (8, 256, 16, 256, 128), (4, 256, 32, 128, 128)],
                         ids=str)
def test_dgrad_rec_after_dual_record(hip_lib, case):
  """stk_conv2d_dgrad_rec_f32 reading the dy record stk_bias_grad_amax_dual_f32 left (the ResnetBlock's last 3x3 conv
  and its 1x1 shortcut peer, graph.py) == stk_conv2d_dgrad_wp_f32 measuring dy itself, bit for bit; and float64."""
  N, Cout, H, Cin3, Cin1 = case
  lib = hip_lib
  _size_gate(lib, 2.0 * N * H * H * Cout * (9 * Cin3 + Cin1))
  d = dev_of(lib)
  alpha = float(np.float32(1 / np.sqrt(2.)))
  dy = rnd(N, Cout, H, H, seed=61)
  w3, w1 = _weights(Cout, Cin3, 3, 0, seed=62), _weights(Cout, Cin1, 1, 0, seed=63)
  dyd = dy.to(d)
  amax3, amax1 = torch.zeros(768, device=d), torch.zeros(768, device=d)
  ws = torch.zeros(N * Cout + 64, device=d)
  db3, db1 = torch.zeros(Cout, device=d), torch.zeros(Cout, device=d)
  call(lib, 'bias_grad_amax_dual_f32', dyd, N, Cout, H * H, alpha, None, 0, db3, amax3[512:], db1, amax1[512:], ws)
  for K, Cin, w, amax in ((3, Cin3, w3, amax3), (1, Cin1, w1, amax1)):
    dims = (N, H, H, Cout, H, H, K, K, 1, K // 2)
    variant = int(lib.conv2d_variant(1, Cin, 0, N, H, H, Cout, H, H, K, K, 1, K // 2, 0))
    if lib.is_device and K == 3:
      assert variant == 5, (K, Cin)       # the 3x3 layer reads the record (the 1x1 peer only on the split kernel)
    fb = int(lib.conv2d_dgrad_ws_bytes(Cin, 0, N, H, H, Cout, K, K, 1, K // 2))
    fws = torch.full((fb // 4 + 64,), float('nan'), device=d)
    wd = w.to(d)
    dx_rec, dx_own = torch.zeros(N, Cin, H, H, device=d), torch.zeros(N, Cin, H, H, device=d)
    call(lib, 'conv2d_dgrad_rec_f32', dyd, wd, 0, dx_rec, Cin, 0.0, None, 0, 0.0, alpha, *dims, None, amax, fws, fb)
    own = torch.full((768,), float('nan'), device=d)
    call(lib, 'conv2d_dgrad_wp_f32', dyd, wd, 0, dx_own, Cin, 0.0, None, 0, 0.0, alpha, *dims, None, own, fws, fb)
    _sync(lib)
    assert torch.equal(dx_rec, dx_own), K
    assert float(amax[512:].max()) == float(dy.abs().max())
    if lib.is_device and variant == 5:
      assert float(own[512:].max()) == float(dy.abs().max())
    ref = torch.nn.grad.conv2d_input((N, Cin, H, H), w.double(), dy.double(), padding=K // 2) * alpha
    _check(f'dgrad_rec {K}x{K} variant {variant} N{N} {Cout}->{Cin} {H}x{H}', {'dx': _err(dx_rec.cpu(), ref)}, PL_DGRAD_RTOL)


def test_gn_param_grad_batch_equals_per_layer_fold(ref_lib, hip_lib):
  """stk_gn_param_grad_batch over descriptors of different C and N == the per-layer fold of stk_gn_bwd_f32, bit for bit
  (include/stk.h: same summation order), and the oracle's fold."""
  layers = [(4, 128, 256, 32), (3, 64, 1024, 32), (7, 256, 64, 32), (2, 512, 16, 32)]     # N, C, HW, G
  max_c = max(c for _, c, _, _ in layers)
  out = {}
  for name, lib in (('ref', ref_lib), ('hip', hip_lib)):
    d = dev_of(lib)
    per_layer, batched, descs, keep = [], [], [], []
    for i, (N, C, HW, G) in enumerate(layers):
      x = (rnd(N, C, HW, seed=70 + i) * 2 + 0.3).to(d)
      dy = rnd(N, C, HW, seed=80 + i).to(d)
      gamma, beta = (rnd(C, seed=90 + i) * 0.5 + 1).to(d), (rnd(C, seed=100 + i) * 0.2).to(d)
      mean, rstd = torch.zeros(N * G, device=d), torch.zeros(N * G, device=d)
      nws = max(int(lib.gn_ws_bytes(N, C, HW, G)) // 4, 2 * N * C) + 64
      ws = torch.zeros(nws, device=d)
      y = torch.zeros(N, C, HW, device=d)
      call(lib, 'gn_fwd_f32', x, C, None, 0, gamma, beta, y, mean, rstd, N, HW, G, 1e-6, 1, 0.0, 1, None, ws)
      dg0, db0 = rnd(C, seed=110 + i).to(d), rnd(C, seed=120 + i).to(d)
      dx = torch.zeros(N, C, HW, device=d)
      dg, db = dg0.clone(), db0.clone()
      call(lib, 'gn_bwd_f32', dy, x, C, None, 0, gamma, beta, mean, rstd, dx, 0.0, None, 0.0, dg, db, ws, N, HW, G, 1, 0.0,
           1, None)
      per_layer.append((dg, db))
      ws2 = torch.zeros(nws, device=d)
      dx2 = torch.zeros(N, C, HW, device=d)
      call(lib, 'gn_bwd_f32', dy, x, C, None, 0, gamma, beta, mean, rstd, dx2, 0.0, None, 0.0, None, None, ws2, N, HW, G, 1,
           0.0, 1, None)
      assert torch.equal(dx, dx2)
      bg, bb = dg0.clone(), db0.clone()
      batched.append((bg, bb))
      descs.append(_GnFoldDesc(ws2.data_ptr(), bg.data_ptr(), bb.data_ptr(), N, C))
      keep += [ws2, x, dy]
    if lib.is_device:
      table = _table(descs, d)
      call(lib, 'gn_param_grad_batch', table, len(descs), max_c)
    else:
      table = (_GnFoldDesc * len(descs))(*descs)
      call(lib, 'gn_param_grad_batch', ctypes.addressof(table), len(descs), max_c)
    _sync(lib)
    if lib.is_device:                # (the checker folds in double either way)
      for (a, b), (c, e) in zip(per_layer, batched):
        assert torch.equal(a, c) and torch.equal(b, e)
    out[name] = [(c.cpu(), e.cpu()) for c, e in batched]
  for (rg, rb), (hg, hb) in zip(out['ref'], out['hip']):
    assert (hg - rg).abs().max().item() <= 2e-5 * rg.abs().max().item()
    assert (hb - rb).abs().max().item() <= 2e-5 * rb.abs().max().item()


GN_BOUND_CASES = [
  # N, C, H, G, act, drop, conv Cout
  (2, 128, 32, 32, 1, 0.0, 128),      # L = 4 x 1024
  (2, 256, 16, 32, 0, 0.1, 256),
  (2, 128, 16, 32, 2, 0.0, 128),
  (2, 256, 8, 32, 3, 0.2, 256),
  (2, 128, 64, 32, 4, 0.1, 128),
  (1, 128, 256, 32, 1, 0.1, 128),     # L = 4 x 65536 = 262144: the 256^2 maps
]


@pytest.mark.parametrize('case', GN_BOUND_CASES, ids=str)
def test_gn_bound_holds_at_the_spike(hip_lib, case):
  """stk_gn_bound_f32 against the largest |y| a group can produce: one spike per group puts |xhat| at ~sqrt(L - 1).
  The bound must hold for every activation code and dropout rate; the planes stk_gn_fwd_pl_f32 writes with it must be
  finite, and a convolution from them must match float64 at the contraction bound.  The group that reaches the bound has
  its spike at the FIRST element of the group, and mean / rstd (y too where there is no dropout) are held to float64 per
  (sample, group) by the metric of tests/_gn_cases.py."""
  N, C, H, G, act, drop, Cout = case
  lib = hip_lib
  HW, L = H * H, C // G * H * H
  _size_gate(lib, 2.0 * N * HW * C * Cout * 9)
  d = dev_of(lib)
  x = torch.zeros(N, C, HW)
  cg = C // G
  for n in range(N):
    for g in range(G):     # one spike per group, at a different place each time; sign and size vary
      x[n, g * cg + (g + n) % cg, (7919 * (g + 3 * n)) % HW] = (1.0 if (g + n) % 2 else -1.0) * (100.0 + g)
  gamma = (rnd(C, seed=131) * 0.5 + 1.0).clamp(-2.4, 2.4)
  g5 = 5 // cg
  c5 = g5 * cg                         # the first channel of the group of channel 5
  gamma[c5] = 2.5                      # the largest |gamma| ...
  beta = (rnd(C, seed=132) * 0.2).clamp(-0.45, 0.45)
  beta[c5] = 0.5                       # ... with the largest |beta| of the same sign on the same channel,
  x[:, g5 * cg:(g5 + 1) * cg] = 0
  x[:, c5, 0] = 1e3                    # whose group's one spike is positive and its FIRST element: y there is the bound up to rounding
  xd, gd, bd = x.to(d), gamma.to(d), beta.to(d)
  rec = torch.full((256,), float('nan'), device=d)
  call(lib, 'gn_bound_f32', gd, bd, C, G, HW, drop, rec)
  ws = torch.zeros(int(lib.gn_ws_bytes(N, C, HW, G)) // 4 + 64, device=d)
  y = torch.zeros(N, C, HW, device=d)
  mean, rstd = torch.zeros(N * G, device=d), torch.zeros(N * G, device=d)
  call(lib, 'gn_fwd_f32', xd, C, None, 0, gd, bd, y, mean, rstd, N, HW, G, 1e-6, act, drop, 99, None, ws)
  stats32 = (mean.clone(), rstd.clone())
  yp = torch.zeros(N, C, HW, device=d)
  rec2 = torch.full((256,), float('nan'), device=d)
  pl = torch.full((int(lib.planes_bytes(N, C, HW)),), 0xAA, dtype=torch.uint8, device=d)
  call(lib, 'gn_fwd_pl_f32', xd, C, None, 0, gd, bd, yp, pl, rec2, mean, rstd, N, HW, G, 1e-6, act, drop, 99, None, ws)
  _sync(lib)
  rec, rec2, y, yp = rec.cpu(), rec2.cpu(), y.cpu(), yp.cpu()
  # against float64, per (sample, group)
  ref = {'y': gc.act_fn(act, F.group_norm(x.double(), G, gamma.double(), beta.double(), gc.EPS))}
  xg = x.double().reshape(N, G, -1)
  ref['mean'] = xg.mean(2)
  ref['rstd'] = (((xg - ref['mean'][:, :, None]) ** 2).mean(2) + gc.EPS).rsqrt()
  for what, yy, (mm, rr) in (('gn_fwd_f32', y, stats32), ('gn_fwd_pl_f32', yp, (mean, rstd))):
    got = {'mean': mm.cpu(), 'rstd': rr.cpu()}
    if drop == 0.0:
      got['y'] = yy
    for k, e in gc.group_errors(got, ref, G).items():
      print(f'  gn spike L={L} {what} {k}: worst per-group error {float(e.max()):.3g}, in the group of the bound {float(e[:, g5].max()):.3g}')
      assert float(e.max()) <= gc.TOL, (what, k, float(e.max()))
  bound = float(rec[0])
  want = (float(gamma.abs().max()) * np.sqrt(L - 1.0) + float(beta.abs().max())) / (1 - drop)
  assert want <= bound <= want * (1 + 2e-5) and float(rec[1:].abs().max()) == 0
  assert torch.equal(rec, rec2)
  top = float(y.abs().max())
  print(f'  gn bound L={L} act={act} p={drop}: max|y| {top:.6g}, bound {bound:.6g}, max|y| / bound {top / bound:.7f}')
  assert top <= bound, (top, bound)
  if drop == 0.0:
    assert top >= 0.99 * bound                 # the spike really reaches the bound
  planes = pl.cpu().numpy().view(np.float16)
  assert np.isfinite(planes).all()
  # a 3x3 convolution from those planes (the next layer of a ResnetBlock)
  w = _weights(Cout, C, 3, 0, seed=133)
  Hs = H
  assert int(lib.conv2d_pl_ok(0, C, 0, N, Hs, Hs, Cout, 3, 3, 1, 1)) == 1
  fb = max(int(lib.conv2d_fwd_ws_bytes(C, 0, N, Hs, Hs, Cout, 3, 3, 1, 1)), 256)
  cws = torch.full((fb // 4 + 64,), float('nan'), device=d)
  out = torch.full((N, Cout, Hs, Hs), float('nan'), device=d)
  call(lib, 'conv2d_fwd_pl_f32', pl, rec2.to(d), C, w.to(d), 0, None, None, 0, None, 1.0, out, N, Hs, Hs, Cout, 3, 3, None,
       cws, fb)
  _sync(lib)
  ref = F.conv2d(yp.reshape(N, C, Hs, Hs).double(), w.double(), padding=1)
  _check(f'conv after gn spike L={L}', {'y': _err(out.cpu(), ref)}, PL_FWD_RTOL)
