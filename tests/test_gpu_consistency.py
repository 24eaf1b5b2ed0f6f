"""The kernels of include/stk_consistency.h (csrc/consistency.hip), the fused consistency loss, the shared dropout seed, the
training step and the consistency sampler built on them, on the device.

The kernels against float64.  The bounds are the rounding model of the header's lines, as in test_gpu_edm.py: every output
element is an expression of rounded products and sums, and forward analysis bounds its error by gamma_k B, where B is the same
expression on absolute values and k the number of roundings on the longest path from an operand to the result, gamma_k = k u /
(1 - k u) < (k + 1) u, u = 2^-24.  The tests hold K = k + 1.  The scalars and the coefficient rows reach the reference as the
fp32 values the kernel receives.

  stk_ct_pair_f32    xin = a y + s n: two products and a sum, k = 2 on the longest path, on |a| |y| + |s| |n|: K_PAIR = 3, at
                     both levels.
  stk_ct_loss_f32    xh = y + sh n: 2;  c_skip xh: 3;  + c_out F: 4 (the other path, c_out F, has 2);  the same for the lower
                     level;  r = fh - fl: 5, on B_r = c_skip_hi (|y| + sh |n|) + c_out_hi |F_hi| + c_skip_lo (|y| + sl |n|) +
                     c_out_lo |F_lo|: K_R = 6.  loss_out is compared with the float64 value lambda S / (sqrt(S + c^2) + c) on
                     the float64 sum S of the SAME fp32 squares (of the r the kernel wrote): the kernel's float64 sum of `inner`
                     non-negative terms in any order differs by at most inner 2^-53 relative; the value is non-decreasing in S
                     with logarithmic derivative in [1/2, 1], so that error passes at most unchanged; c c, the sum, the root, h +
                     c, lambda S, the quotient and the division by inner add one 2^-53 each (7, each passing with a factor <= 1),
                     and the result is rounded to fp32 once: |loss - want| <= (2^-24 + (inner + 8) 2^-53) want, held with the
                     factor 1 + 2^-20 that covers the second-order terms.  gfac_out = lambda c_out_hi / sqrt(S + c^2) (/ inner):
                     the root halves the error of S, and c c, the sum, the root, the product, the quotient and the division are
                     6 roundings: (2^-24 + (inner + 8) 2^-53) |want| holds it as well.
  stk_ct_loss_grad_f32  k = gfac dloss: 1;  dF = k r: 2, on |k| |r|: K_G = 3.
  stk_ct_step_f32    x0 = cs x + co F: k = 2 on B_0 = |cs| |x| + |co| |F|; the clamp is monotone and 1-Lipschitz, it rounds
                     nothing and widens no error: K_X0 = 3.  x_out = x0 + c_z z: the third rounding, on B_x = B_0 + |c_z| |z|:
                     K_X = 4.  xin_out = c_in_next x_out: K_XIN = 5 on |c_in_next| B_x.

Besides the bounds every output is compared BIT FOR BIT with a numpy float32 restatement of the header's lines (numpy rounds
each operation once and fuses nothing), and every in-place / NULL form the header allows with the separate-buffer form.

stk_ct_coeffs_f32: the eight algebraic rows and lambda are float64 expressions of correctly rounded operations rounded to fp32
once, so numpy float64 in the same order reproduces them bit for bit; the logarithm is not correctly rounded in either
library, so the two c_noise rows are held to one fp32 unit in the last place.

Fused against torch-expression loss on the tiny networks: each path's losses and network-output gradient are held to the
kernel bounds around the float64 restatement on ITS OWN network outputs (as test_gpu_edm.py holds the EDM pair: dr = K_R u B_r
per element, dS = sum 2 |r| dr + dr^2, and the loss moves by at most lambda dS / (2 sqrt(S - dS + c^2))); the flat parameter
gradients of the two paths, which the engine's fp32 backward produces from those two output gradients, are held to 1e-5 of the
largest entry -- the figure _model_cases.fused_loss_matches_torch holds for the same A/B of the Soft-Truncation loss.

The sampler with the closed-form network against the float64 restatement: the tolerance is measured, not fixed in advance --
the restatement is run again in numpy fp32, and four times its deviation from float64 is what the product loop may deviate.
"""
import copy
import sys

import numpy as np
import pytest
import torch

import _consistency_ref as R
from _model_util import Tap as _Tap, make_state, patched_rng, randomize_, tiny_config
from _stream_util import ROW_SHAPES, SHAPES, U, case_id, drawn_operands, nan as _nan, place, ptr as _ptr, stream as _stream, within

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file, worst case over the shapes, in units of u B against the bound held:
stk_ct_pair_f32 1.97 (3);  stk_ct_loss_f32 r_out 2.63 (6), loss_out 0.98 and gfac_out 0.98 of their bound (3000 rows of 4: a
half-unit rounding to fp32 is the whole bound), stk_ct_loss_grad_f32 dF 1.93 (3);  stk_ct_step_f32 x0_out 1.98 (3), x_out 2.82
(4), xin_out 3.34 (5);  c_noise differs from numpy in 0 of 3329 levels, both rows.  Fused and torch-expression loss on the tiny
networks: losses 0.011 (vp) / 0.025 (ve) of their bound, the network-output gradient 0.20-0.21, both paths alike; the flat
parameter gradients of the two paths differ by 1.1e-7 ... 2.0e-7 of the largest entry (bound 1e-5).  Shared mask: two
evaluations under one pinned seed are bit-equal with dropout 0.3 as with dropout 0; two seeds differ in 0.999 of the elements.
Closed-form sampler: the product loop deviates 1.32e-7 (1 step) / 1.35e-7 (3 steps) / 1.82e-7 (3 steps, clamped) from the
float64 restatement, the numpy fp32 restatement 1.12e-7 / 1.49e-7 / 1.90e-7; one step against the exact flow 1.49e-7."""

K_PAIR, K_R, K_G = 3, 6, 3
K_X0, K_X, K_XIN = 3, 4, 5
S_DATA, S_MIN, S_MAX = 0.5, 0.002, 80.
E32 = float(np.float32(S_MIN))
EINVAL, EUNSUPPORTED = -1, -3
INF = float('inf')
f32 = lambda v: float(np.float32(v))
@pytest.fixture(scope='module')
def operands():
  """Four fp32 tensors per shape on the host (numpy), drawn once: x / y, z / n, F / F_hi, F_lo."""
  return drawn_operands()


def _pairs(B):
  """B pairs sigma_hi > sigma_lo (fp32) over the training range: narrow and wide gaps, and -- when there is room -- the lowest
  pair of the 1281-level grid, whose lower level is sigma_min (c_skip = 1, c_out = 0), and the pair that ends in sigma_max."""
  rng = np.random.RandomState(B)
  lo = np.exp(rng.uniform(np.log(0.003), np.log(60.), size=B)).astype(np.float32)
  hi = (lo.astype(np.float64) * (1. + np.exp(rng.uniform(np.log(1e-3), np.log(0.5), size=B)))).astype(np.float32)
  if B >= 2:
    grid = R.levels(S_MIN, S_MAX, 1281)
    lo[0], hi[0] = grid[0], grid[1]
    lo[-1], hi[-1] = grid[-2], grid[-1]
  assert bool((hi > lo).all())
  return hi, lo


def _coeffs(lib, hi, lo, dev):
  B = hi.shape[0]
  hd, ld = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
  coef = torch.full((11, B), float('nan'), device=dev)
  lib.ct_coeffs_f32(hd.data_ptr(), ld.data_ptr(), S_DATA, S_MIN, coef.data_ptr(), B, _stream())
  return hd, ld, coef


# ---- stk_ct_coeffs_f32 --------------------------------------------------------------------------------------------------
def test_coeffs_are_the_float64_expressions(hip_lib):
  dev = torch.device('cuda:0')
  grid = R.levels(S_MIN, S_MAX, 1281).astype(np.float32)
  sweep = np.exp(np.linspace(np.log(0.0021), np.log(79.), 2048)).astype(np.float32)
  hi = np.concatenate([grid[1:], sweep * np.float32(1.25), [1.0]]).astype(np.float32)
  lo = np.concatenate([grid[:-1], sweep, [0.5]]).astype(np.float32)
  _, _, coef = _coeffs(hip_lib, hi, lo, dev)
  got = coef.cpu().numpy()
  want = R.coeff_rows(hi, lo, S_DATA, S_MIN, np.float32)
  names = ('c_in', 'c_in sigma', 'c_skip', 'c_out', 'c_noise')
  for k in range(11):
    name = 'lambda' if k == 10 else names[k % 5] + (' hi' if k < 5 else ' lo')
    if k in (4, 9):
      ulp = np.spacing(np.abs(want[k]))
      off = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)) / np.maximum(ulp, np.float32(1e-45))
      print(f'{name}: {int((got[k] != want[k]).sum())} of {hi.size} differ from numpy, worst {off.max():.1f} ulp')
      assert bool((off <= 1.).all()), name
    else:
      assert np.array_equal(got[k], want[k]), f'{name}: {int((got[k] != want[k]).sum())} of {hi.size} differ from numpy float64'
  # the boundary condition, exactly, at the lowest level of the grid; and the papers' formulas
  assert got[7][0] == 1. and got[8][0] == 0.
  c_in, c_skip, c_out, _ = R.boundary(hi.astype(np.float64), S_DATA, E32)
  for k, ref in ((0, c_in), (2, c_skip), (3, c_out)):
    assert np.allclose(got[k], ref, rtol=2e-7, atol=0), k
  # a level the logarithm or the quotients cannot take yields NaN or inf in its columns only
  bad_hi = np.array([1., 0., -1., np.inf, np.nan, 2., 3.], dtype=np.float32)
  bad_lo = np.array([.5, .5, .5, .5, .5, 2., 1.], dtype=np.float32)
  _, _, bad = _coeffs(hip_lib, bad_hi, bad_lo, dev)
  bad = bad.cpu().numpy()
  assert np.isfinite(bad[:, [0, 6]]).all() and not np.isfinite(bad[:, 1:5]).all(axis=0).any()
  assert np.isinf(bad[10, 5]) and np.isfinite(bad[:10, 5]).all(), 'equal levels: an infinite lambda and nothing else'


# ---- stk_ct_pair_f32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,shifted', ROW_SHAPES, ids=case_id)
def test_pair_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  y, n = operands[shape][:2]
  B, inner = shape[0], int(np.prod(shape[1:]))
  hi, lo = _pairs(B)
  _, _, coef = _coeffs(hip_lib, hi, lo, dev)
  rows = coef.cpu().numpy()
  w = lambda v, dt: v.astype(dt).reshape(B, 1, 1, 1)
  yd, nd = place(y, dev, shifted), place(n, dev, shifted)
  out_h, out_l = _nan(shape, dev, shifted), _nan(shape, dev, shifted)
  hip_lib.ct_pair_f32(yd.data_ptr(), nd.data_ptr(), coef.data_ptr(), out_h.data_ptr(), out_l.data_ptr(), B, inner, _stream())
  y64, n64 = y.astype(np.float64), n.astype(np.float64)
  what = f'ct_pair {shape} shifted={shifted}'
  worst = 0.
  for out, a, s, name in ((out_h, rows[0], rows[1], 'xin_hi'), (out_l, rows[5], rows[6], 'xin_lo')):
    want = w(a, np.float64) * y64 + w(s, np.float64) * n64
    mag = w(a, np.float64) * np.abs(y64) + w(s, np.float64) * np.abs(n64)
    worst = max(worst, within(out, want, mag, K_PAIR, f'{what} {name}'))
    assert np.array_equal(out.cpu().numpy(), w(a, np.float32) * y + w(s, np.float32) * n), f'{what}: {name} is not the fp32 restatement'
  assert np.array_equal(yd.cpu().numpy(), y) and np.array_equal(nd.cpu().numpy(), n), what + ': an operand was written'
  # ... which is what two stk_perturb_f32 launches of stk.h write
  two = _nan(shape, dev, shifted)
  hip_lib.perturb_f32(yd.data_ptr(), nd.data_ptr(), coef[5].data_ptr(), coef[6].data_ptr(), two.data_ptr(), B, inner, _stream())
  assert torch.equal(two, out_l)
  print(f'{what}: worst {worst:.2f} u B (bound {K_PAIR})')


# ---- stk_ct_loss_f32 / stk_ct_loss_grad_f32 ---------------------------------------------------------------------------------
def _loss(lib, Fh, Fl, y, n, hd, ld, coef, c, r_out, gfac_out, loss_out, reduce_mean, ws=None):
  B, inner = y.shape[0], y[0].numel()
  if ws is None:
    ws = torch.empty(int(lib.ct_ws_bytes(B, inner)), dtype=torch.uint8, device=y.device)
  lib.ct_loss_f32(Fh.data_ptr(), Fl.data_ptr(), y.data_ptr(), n.data_ptr(), hd.data_ptr(), ld.data_ptr(), coef.data_ptr(), c,
                  ws.data_ptr(), ws.numel(), _ptr(r_out), _ptr(gfac_out), loss_out.data_ptr(), B, inner, int(reduce_mean), _stream())


@pytest.mark.parametrize('shape,shifted', ROW_SHAPES, ids=case_id)
def test_loss_pair_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  y, n, Fh, Fl = operands[shape]
  B, inner = shape[0], int(np.prod(shape[1:]))
  hi, lo = _pairs(B)
  hd, ld, coef = _coeffs(hip_lib, hi, lo, dev)
  rows = coef.cpu().numpy()
  w = lambda v, dt: v.astype(dt).reshape(B, 1, 1, 1)
  yd, nd, Fhd, Fld = (place(t, dev, shifted) for t in (y, n, Fh, Fl))
  what = f'ct_loss {shape} shifted={shifted}'
  c = f32(0.00054 * np.sqrt(inner))
  y64, n64, Fh64, Fl64 = (t.astype(np.float64) for t in (y, n, Fh, Fl))
  d = np.float64
  want_r = ((w(rows[2], d) * (y64 + w(hi, d) * n64) + w(rows[3], d) * Fh64)
            - (w(rows[7], d) * (y64 + w(lo, d) * n64) + w(rows[8], d) * Fl64))
  mag_r = (w(rows[2], d) * (np.abs(y64) + w(hi, d) * np.abs(n64)) + w(rows[3], d) * np.abs(Fh64)
           + w(rows[7], d) * (np.abs(y64) + w(lo, d) * np.abs(n64)) + w(rows[8], d) * np.abs(Fl64))
  s = np.float32
  bits_r = ((w(rows[2], s) * (y + w(hi, s) * n) + w(rows[3], s) * Fh) - (w(rows[7], s) * (y + w(lo, s) * n) + w(rows[8], s) * Fl))
  assert bits_r.dtype == np.float32
  S = (bits_r * bits_r).astype(np.float64).reshape(B, -1).sum(axis=1)          # the SAME fp32 squares, summed in float64
  L, C = rows[10].astype(np.float64), float(c)
  h = np.sqrt(S + C * C)
  go = np.random.RandomState(3).standard_normal(B).astype(np.float32)
  go_d = torch.from_numpy(go).to(dev)
  rel_tol = (2. ** -24 + (inner + 8) * 2. ** -53) * (1 + 2. ** -20)
  for reduce_mean in (False, True):
    r_out, gfac, loss_out = _nan(shape, dev, shifted), torch.full((B,), float('nan'), device=dev), torch.full((B,), float('nan'), device=dev)
    _loss(hip_lib, Fhd, Fld, yd, nd, hd, ld, coef, c, r_out, gfac, loss_out, reduce_mean)
    w_r = within(r_out, want_r, mag_r, K_R, what + ' r_out')
    assert np.array_equal(r_out.cpu().numpy(), bits_r), what + ': r_out is not the fp32 restatement bit for bit'
    want_l, want_f = (L * S) / (h + C), (L * rows[3].astype(np.float64)) / h
    if reduce_mean:
      want_l, want_f = want_l / inner, want_f / inner
    got_l, got_f = loss_out.cpu().double().numpy(), gfac.cpu().double().numpy()
    assert np.isfinite(got_l).all() and np.isfinite(got_f).all() and bool((got_l >= 0).all())
    worst_l = float((np.abs(got_l - want_l) / np.maximum(rel_tol * want_l, 1e-300)).max())
    worst_f = float((np.abs(got_f - want_f) / np.maximum(rel_tol * np.abs(want_f), 1e-300)).max())
    assert bool((np.abs(got_l - want_l) <= rel_tol * want_l).all()), f'{what} reduce_mean={reduce_mean}: loss_out off by {worst_l:.2f} of its bound'
    assert bool((np.abs(got_f - want_f) <= rel_tol * np.abs(want_f)).all()), f'{what} reduce_mean={reduce_mean}: gfac_out off by {worst_f:.2f} of its bound'
    # run to run, and without the residual: the same bits
    again, no_r = torch.full((B,), float('nan'), device=dev), torch.full((B,), float('nan'), device=dev)
    r_again, f_again = _nan(shape, dev, shifted), torch.full((B,), float('nan'), device=dev)
    _loss(hip_lib, Fhd, Fld, yd, nd, hd, ld, coef, c, r_again, f_again, again, reduce_mean)
    _loss(hip_lib, Fhd, Fld, yd, nd, hd, ld, coef, c, None, None, no_r, reduce_mean)
    assert torch.equal(again, loss_out) and torch.equal(r_again, r_out) and torch.equal(f_again, gfac), what + ': not reproducible'
    assert torch.equal(no_r, loss_out), what + ': the form without the residual gives other bits'
    # the gradient on the residual and the factor the forward kept
    f_np = gfac.cpu().numpy()
    k32 = f_np * go
    k64 = f_np.astype(np.float64) * go.astype(np.float64)
    dF = _nan(shape, dev, shifted)
    grad = lambda r_, out_: hip_lib.ct_loss_grad_f32(r_.data_ptr(), gfac.data_ptr(), go_d.data_ptr(), out_.data_ptr(), B, inner, _stream())
    grad(r_out, dF)
    r64 = bits_r.astype(np.float64)
    w_g = within(dF, w(k64, d) * r64, np.abs(w(k64, d) * r64), K_G, what + ' dF')
    assert np.array_equal(dF.cpu().numpy(), w(k32, s) * bits_r), what + ': dF is not the fp32 restatement bit for bit'
    assert np.array_equal(r_out.cpu().numpy(), bits_r), 'the residual was written'
    grad(r_out, r_out)                                   # in place
    assert torch.equal(r_out, dF), what + ': dF = r differs from the separate-buffer form'
    print(f'{what} reduce_mean={reduce_mean}: worst r_out {w_r:.2f} u B (bound {K_R}), loss_out {worst_l:.2f} and gfac_out '
          f'{worst_f:.2f} of their bound, dF {w_g:.2f} u B (bound {K_G})')
  for t_d, t_h in ((yd, y), (nd, n), (Fhd, Fh), (Fld, Fl)):
    assert np.array_equal(t_d.cpu().numpy(), t_h), what + ': an operand was written'


# ---- stk_ct_step_f32 ----------------------------------------------------------------------------------------------------
# (cs, co, lo, hi, c_z, c_in_next): the step at 80 towards 0.821 with the data-range clamp; the same without a clamp
STEP_ROWS = [tuple(f32(v) for v in (3.9e-5, 0.49998, -1., 1., 0.821, 1.0403)), tuple(f32(v) for v in (0.27, 0.426, -INF, INF, 0.05, 1.99))]


def _step_restate(x, F, z, row, dtype):
  cs, co, lo, hi, cz, cn = (dtype(v) for v in row)
  x, F = x.astype(dtype), F.astype(dtype)
  x0 = cs * x + co * F
  x0 = np.where(x0 < lo, lo, x0)
  x0 = np.where(x0 > hi, hi, x0)
  b0 = abs(cs) * np.abs(x) + abs(co) * np.abs(F)
  if z is None:
    return x0, None, None, b0, None
  z = z.astype(dtype)
  xo = x0 + cz * z
  return x0, xo, cn * xo, b0, b0 + abs(cz) * np.abs(z)


def _step(lib, x, F, z, row, x0_out, x_out, xin_out):
  lib.ct_step_f32(x.data_ptr(), F.data_ptr(), _ptr(z), *row, _ptr(x0_out), _ptr(x_out), _ptr(xin_out), x.numel(), _stream())


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_step_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  x, z, F, _ = operands[shape]
  worst = dict(x0=0., x=0., xin=0.)
  for row in STEP_ROWS:
    xd, zd, Fd = (place(t, dev, shifted) for t in (x, z, F))
    want = _step_restate(x, F, z, row, np.float64)
    bits = _step_restate(x, F, z, row, np.float32)
    what = f'ct_step {shape} shifted={shifted} clamp={row[2]}'
    x0, xo, xin = (_nan(shape, dev, shifted) for _ in range(3))
    _step(hip_lib, xd, Fd, zd, row, x0, xo, xin)
    worst['x0'] = max(worst['x0'], within(x0, want[0], want[3], K_X0, what + ' x0_out'))
    worst['x'] = max(worst['x'], within(xo, want[1], want[4], K_X, what + ' x_out'))
    worst['xin'] = max(worst['xin'], within(xin, want[2], abs(row[5]) * want[4], K_XIN, what + ' xin_out'))
    for got, ref, name in ((x0, bits[0], 'x0_out'), (xo, bits[1], 'x_out'), (xin, bits[2], 'xin_out')):
      assert np.array_equal(got.cpu().numpy(), ref), f'{what}: {name} is not the fp32 restatement bit for bit'
    if row[2] == -1. and x.size >= 300:
      assert float(x0.min()) >= -1. and float(x0.max()) <= 1. and bool((x0.abs() == 1.).any()), what + ': the clamp did not act'
    for t_d, t_h in ((xd, x), (zd, z), (Fd, F)):
      assert np.array_equal(t_d.cpu().numpy(), t_h), what + ': an operand was written'
    # without x0_out: the other outputs keep their bits
    xo2, xin2 = _nan(shape, dev, shifted), _nan(shape, dev, shifted)
    _step(hip_lib, xd, Fd, zd, row, None, xo2, xin2)
    assert torch.equal(xo2, xo) and torch.equal(xin2, xin), what
    # the last step (z NULL): only x0_out is written, with the same bits; x_out and xin_out are not touched, given or not
    last, keep_a, keep_b = _nan(shape, dev, shifted), torch.full(shape, 7.0, device=dev), torch.full(shape, 7.0, device=dev)
    _step(hip_lib, xd, Fd, None, row, last, keep_a, keep_b)
    assert torch.equal(last, x0) and bool((keep_a == 7.0).all()) and bool((keep_b == 7.0).all()), what
    last2 = _nan(shape, dev, shifted)
    _step(hip_lib, xd, Fd, None, row, last2, None, None)
    assert torch.equal(last2, x0), what
    # in place: x_out = x;  x0_out = x on the last step;  x0_out = x with x_out elsewhere
    xa, xi = place(x, dev, shifted), _nan(shape, dev, shifted)
    _step(hip_lib, xa, Fd, zd, row, None, xa, xi)
    assert torch.equal(xa, xo) and torch.equal(xi, xin), what + ': x_out = x differs from the separate-buffer form'
    xa = place(x, dev, shifted)
    _step(hip_lib, xa, Fd, None, row, xa, None, None)
    assert torch.equal(xa, x0), what + ': x0_out = x differs from the separate-buffer form'
    xa, xo3, xi = place(x, dev, shifted), _nan(shape, dev, shifted), _nan(shape, dev, shifted)
    _step(hip_lib, xa, Fd, zd, row, xa, xo3, xi)
    assert torch.equal(xa, x0) and torch.equal(xo3, xo) and torch.equal(xi, xin), what
  print(f'ct_step {shape} shifted={shifted}: worst x0_out {worst["x0"]:.2f} u B (bound {K_X0}), x_out {worst["x"]:.2f} ({K_X}), '
        f'xin_out {worst["xin"]:.2f} ({K_XIN})')


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(hip_lib):
  """Every refusal of the header returns before any launch: the outputs keep their sentinel."""
  dev = torch.device('cuda:0')
  B, shape = 2, (2, 3, 4, 4)
  inner, n = 48, 96
  a, b, c, d = (torch.randn(shape, device=dev) for _ in range(4))
  outs = [torch.full(shape, 7.0, device=dev) for _ in range(3)]
  hi, lo = torch.tensor([0.6, 2.], device=dev), torch.tensor([0.5, 1.], device=dev)
  coef, loss, gf, go = (torch.full((11, B), 7.0, device=dev), torch.full((B,), 7.0, device=dev), torch.full((B,), 7.0, device=dev),
                        torch.ones(B, device=dev))
  ws_bytes = int(hip_lib.ct_ws_bytes(B, inner))
  assert ws_bytes == B * 8
  ws = torch.full((ws_bytes // 8 + 1,), 7.0, dtype=torch.float64, device=dev)
  nan, inf = float('nan'), INF
  s = _stream()

  def clean():
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [coef, loss, gf, ws]), 'a refused call wrote'

  def step(x=a, F=b, z=c, lo_=-1., hi_=1., x0=outs[0], xo=outs[1], xin=outs[2], n=n):
    code = hip_lib.ct_step_f32.raw(_ptr(x), _ptr(F), _ptr(z), 0.04, 0.49, lo_, hi_, 0.8, 1.04, _ptr(x0), _ptr(xo), _ptr(xin), n, s)
    clean()
    return code

  assert step(x=None) == EINVAL and step(F=None) == EINVAL and step(xo=None) == EINVAL and step(xin=None) == EINVAL
  assert step(z=None, x0=None) == EINVAL
  assert step(n=0) == EINVAL and step(n=-4) == EINVAL
  assert step(lo_=1., hi_=-1.) == EINVAL and step(lo_=nan) == EINVAL and step(hi_=nan) == EINVAL
  assert step(n=2 ** 31) == EUNSUPPORTED and step(n=2 ** 40) == EUNSUPPORTED

  def coeffs(h=hi, l=lo, s_data=0.5, s_min=0.002, out=coef, B=B):
    code = hip_lib.ct_coeffs_f32.raw(_ptr(h), _ptr(l), s_data, s_min, _ptr(out), B, s)
    clean()
    return code

  assert coeffs(h=None) == EINVAL and coeffs(l=None) == EINVAL and coeffs(out=None) == EINVAL
  assert coeffs(B=0) == EINVAL and coeffs(B=-1) == EINVAL
  assert coeffs(s_data=0.) == EINVAL and coeffs(s_data=-0.5) == EINVAL and coeffs(s_data=nan) == EINVAL and coeffs(s_data=inf) == EINVAL
  assert coeffs(s_min=-0.1) == EINVAL and coeffs(s_min=nan) == EINVAL and coeffs(s_min=inf) == EINVAL
  good = torch.empty((11, B), device=dev)
  hip_lib.ct_coeffs_f32(hi.data_ptr(), lo.data_ptr(), 0.5, 0.002, good.data_ptr(), B, s)

  def pair(y=a, n_=b, cf=good, oh=outs[0], ol=outs[1], B=B, inner=inner):
    code = hip_lib.ct_pair_f32.raw(_ptr(y), _ptr(n_), _ptr(cf), _ptr(oh), _ptr(ol), B, inner, s)
    clean()
    return code

  for key in ('y', 'n_', 'cf', 'oh', 'ol'):
    assert pair(**{key: None}) == EINVAL, key
  assert pair(B=0) == EINVAL and pair(inner=0) == EINVAL and pair(B=2, inner=2 ** 30) == EUNSUPPORTED and pair(B=1, inner=2 ** 31) == EUNSUPPORTED

  def lossf(Fh=a, Fl=b, y=c, n_=d, h=hi, l=lo, cf=good, cc=0.004, w=ws, wb=ws_bytes, r=outs[0], g=gf, out=loss, B=B, inner=inner):
    code = hip_lib.ct_loss_f32.raw(_ptr(Fh), _ptr(Fl), _ptr(y), _ptr(n_), _ptr(h), _ptr(l), _ptr(cf), cc, _ptr(w), wb, _ptr(r), _ptr(g),
                                   _ptr(out), B, inner, 0, s)
    clean()
    return code

  for key in ('Fh', 'Fl', 'y', 'n_', 'h', 'l', 'cf', 'w', 'out'):
    assert lossf(**{key: None}) == EINVAL, key
  assert lossf(r=None) == EINVAL and lossf(g=None) == EINVAL, 'r_out and gfac_out are NULL together or not at all'
  assert lossf(cc=0.) == EINVAL and lossf(cc=-1.) == EINVAL and lossf(cc=nan) == EINVAL and lossf(cc=inf) == EINVAL
  assert lossf(B=0) == EINVAL and lossf(inner=0) == EINVAL and lossf(wb=ws_bytes - 1) == EINVAL
  misaligned = hip_lib.ct_loss_f32.raw(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), hi.data_ptr(), lo.data_ptr(),
                                       good.data_ptr(), 0.004, ws.data_ptr() + 4, ws_bytes, outs[0].data_ptr(), gf.data_ptr(),
                                       loss.data_ptr(), B, inner, 0, s)
  clean()
  assert misaligned == EINVAL
  assert lossf(B=2, inner=2 ** 30) == EUNSUPPORTED and lossf(B=1, inner=2 ** 31) == EUNSUPPORTED

  def gradf(r=a, g=go, dl=go, out=outs[0], B=B, inner=inner):
    code = hip_lib.ct_loss_grad_f32.raw(_ptr(r), _ptr(g), _ptr(dl), _ptr(out), B, inner, s)
    clean()
    return code

  for key in ('r', 'g', 'dl', 'out'):
    assert gradf(**{key: None}) == EINVAL, key
  assert gradf(B=0) == EINVAL and gradf(inner=-1) == EINVAL and gradf(B=2, inner=2 ** 30) == EUNSUPPORTED
  # ... and the accepted edge forms run
  assert step(z=None, x0=torch.empty_like(a), xo=None, xin=None) == 0
  assert step(x0=None, xo=torch.empty_like(a), xin=torch.empty_like(a)) == 0
  assert step(lo_=-inf, hi_=inf, x0=torch.empty_like(a), xo=torch.empty_like(a), xin=torch.empty_like(a)) == 0
  assert lossf(r=None, g=None, out=torch.empty(B, device=dev), w=torch.empty(ws_bytes, dtype=torch.uint8, device=dev)) == 0
  # the checked binding raises the package's error
  with pytest.raises(RuntimeError, match='stk_ct_step_f32 failed'):
    hip_lib.ct_step_f32(a.data_ptr(), b.data_ptr(), None, 0.04, 0.49, -1., 1., 0., 0., None, None, None, n, s)


# ---- the fused loss against the torch-expression loss ---------------------------------------------------------------------
_built = {}


def _model(st, base, lib, seed=0):
  """(cfg, sde, model): the product model of `base` on the device with randomised weights (no oracle twin)."""
  cfg = copy.deepcopy(base)
  cfg.device = torch.device('cuda:0')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(seed)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  net = net.to(cfg.device)
  randomize_(net, seed)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  return cfg, sde, model


def _tiny(st, lib, family, dropout=0.0, num_classes=0, **ct):
  """(cfg, sde, model) of a tiny network under configs.consistency, in eval mode: built once per variant."""
  key = (family, dropout, num_classes, tuple(sorted(ct.items())))
  if key not in _built:
    base = st.configs.consistency(tiny_config(st, family, dropout=dropout), **ct)
    if num_classes:
      base.model.num_classes = num_classes
    cfg, sde, model = _model(st, base, lib)
    model.eval()
    _built[key] = (cfg, sde, model)
  return _built[key]


@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_fused_loss_matches_the_torch_expressions(st, hip_lib, family, reduce_mean):
  """Same levels and the same n (one CPU stream serves both paths): each path's losses and network-output gradient lie
  within the kernel bounds of the float64 restatement on ITS OWN network outputs; the flat parameter gradients of the two
  paths agree to 1e-5 of the largest entry (module docstring)."""
  cfg, sde, model = _tiny(st, hip_lib, family)
  cfg = copy.deepcopy(cfg)
  cfg.training.reduce_mean = reduce_mean
  dev = cfg.device
  B = 6
  batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(3)).to(dev)
  inner = batch[0].numel()
  loss_fn = st.losses.get_consistency_loss_fn(cfg, sde, True)
  grid = R.levels(S_MIN, S_MAX, 11)
  idx = np.array([0, 3, 5, 7, 8, 9])
  lo, hi = grid[idx], grid[idx + 1]
  levels = (torch.tensor(hi, dtype=torch.float32), torch.tensor(lo, dtype=torch.float32))
  go = torch.randn(B, generator=torch.Generator().manual_seed(4)).to(dev)
  with patched_rng(17):
    n = torch.randn_like(batch).cpu().double().numpy()
  rows = R.coeff_rows(hi, lo, S_DATA, S_MIN, np.float32).astype(np.float64)
  y = batch.cpu().double().numpy()
  w = lambda v: v.reshape(B, 1, 1, 1)
  c = f32(0.00054 * np.sqrt(inner))
  calls = []
  saved_fused, saved_entry = st.losses.FUSED_LOSS, hip_lib.ct_loss_f32
  hip_lib.ct_loss_f32 = lambda *a: (calls.append('loss'), saved_entry(*a))[1]
  seen, flat = {}, {}
  try:
    for fused in (True, False):
      st.losses.FUSED_LOSS = fused
      tap = _Tap(model)
      model.zero_grad()
      with patched_rng(17):
        losses = loss_fn(tap, batch, levels=levels)
      (losses * go).sum().backward()
      assert calls == ['loss'], f'fused={fused}: stk_ct_loss_f32 ran {len(calls)} times so far'
      (xin_lo, cond_lo, F_lo, g_lo), (xin_hi, cond_hi, F_hi, g_hi) = tap.seen
      assert g_lo is False and g_hi is True and not F_lo.requires_grad, 'the target runs first and without gradient'
      seen[fused] = (xin_hi, cond_hi, xin_lo, cond_lo)
      flat[fused] = torch.cat([p.grad.detach().reshape(-1) for p in model.parameters() if p.grad is not None]).cpu().double()
      Fh, Fl = F_hi.detach().cpu().double().numpy(), F_lo.cpu().double().numpy()
      r = (w(rows[2]) * (y + w(hi) * n) + w(rows[3]) * Fh) - (w(rows[7]) * (y + w(lo) * n) + w(rows[8]) * Fl)
      mag = (w(rows[2]) * (np.abs(y) + w(hi) * np.abs(n)) + w(rows[3]) * np.abs(Fh)
             + w(rows[7]) * (np.abs(y) + w(lo) * np.abs(n)) + w(rows[8]) * np.abs(Fl))
      dr = K_R * U * mag
      scale = 1. / inner if reduce_mean else 1.
      S = (r * r).reshape(B, -1).sum(axis=1)
      dS = (2 * np.abs(r) * dr + dr * dr).reshape(B, -1).sum(axis=1)
      S_lo = np.maximum(S - dS, 0.)
      L = rows[10]
      want = L * S / (np.sqrt(S + c * c) + c) * scale
      tol = L * dS / (2 * np.sqrt(S_lo + c * c)) * scale + (2. ** -23 + (inner + 8) * 2. ** -53) * want
      got = losses.detach().cpu().double().numpy()
      worst = float((np.abs(got - want) / tol).max())
      k = L * rows[3] / np.sqrt(S + c * c) * go.cpu().double().numpy() * scale
      k_rel = dS / (2 * (S_lo + c * c)) + 2. ** -23         # the factor: half the relative error of S + c^2, rounded to fp32
      g_tol = np.abs(w(k)) * (dr + (w(k_rel) + K_G * U) * (np.abs(r) + dr))
      g_err = np.abs(F_hi.grad.cpu().double().numpy() - w(k) * r)
      print(f'{family} reduce_mean={reduce_mean} fused={fused}: loss {worst:.3f} of its bound, dLoss/dF '
            f'{float((g_err / g_tol).max()):.3f} of its bound')
      assert bool((np.abs(got - want) <= tol).all()) and bool((g_err <= g_tol).all())
  finally:
    st.losses.FUSED_LOSS, hip_lib.ct_loss_f32 = saved_fused, saved_entry
  e_flat = float((flat[True] - flat[False]).abs().max() / flat[False].abs().max())
  print(f'{family} reduce_mean={reduce_mean}: flat parameter gradients of the two paths differ by {e_flat:.2e} of the largest entry (bound 1e-5)')
  assert float(flat[False].abs().max()) > 0 and e_flat <= 1e-5
  # the network inputs of the two paths: to the rounding of c_in y + (c_in sigma) n, c_noise to one unit in the last place
  for fused in (True, False):
    for xin, cond, base in ((seen[fused][0], seen[fused][1], 0), (seen[fused][2], seen[fused][3], 5)):
      x_want = w(rows[base]) * y + w(rows[base + 1]) * n
      x_mag = w(rows[base]) * np.abs(y) + w(rows[base + 1]) * np.abs(n)
      within(xin, x_want, x_mag, 4, f'{family} fused={fused} x_in')
      want_cond = np.exp(rows[base + 4]) if cfg.model.embedding_type == 'fourier' else rows[base + 4]
      assert np.allclose(cond.cpu().double().numpy(), want_cond, rtol=4 * U, atol=4e-8)


# ---- the shared dropout mask ------------------------------------------------------------------------------------------------
def test_one_seed_gives_both_evaluations_one_mask(st, hip_lib):
  dev = torch.device('cuda:0')
  x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev) * 2
  sigma = torch.tensor([0.01, 0.5, 3., 60.], device=dev)
  dev_of = {}
  for dropout in (0.0, 0.3):
    cfg, sde, model = _tiny(st, hip_lib, 'vp', dropout=dropout)
    f = st.models.utils.get_consistency_fn(cfg, sde, model, train=True)
    ex = model.module.engine()
    with torch.no_grad():
      with ex.dropout_seed(1234):
        a, b, c3 = f(x, sigma), f(x, sigma), f(x, sigma)     # the third runs as a graph replay where graphs are on
      with ex.dropout_seed(99):
        other = f(x, sigma)
    model.eval()
    dev_of[dropout] = max(float((a - b).abs().max()), float((a - c3).abs().max()))
    if dropout:
      differ = float((a != other).float().mean())
      print(f'dropout {dropout}: two seeds differ in {differ:.3f} of the elements')
      assert differ > 0.5, 'two seeds gave (nearly) the same masks'
  print(f'two evaluations under one seed deviate {dev_of[0.3]:.3e} with dropout 0.3, {dev_of[0.0]:.3e} with dropout 0')
  if dev_of[0.0] == 0.:
    assert dev_of[0.3] == 0., 'the evaluations are bit-equal without dropout and not with a pinned seed'
  else:
    assert dev_of[0.3] <= 4 * dev_of[0.0]


def test_loss_runs_both_evaluations_under_the_drawn_seed(st, hip_lib):
  cfg, sde, model = _tiny(st, hip_lib, 'vp', dropout=0.3, s0=2, s1=8)
  ex = model.module.engine()
  loss_fn = st.losses.get_consistency_loss_fn(cfg, sde, True)
  batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(3)).to(cfg.device)
  seeds = []
  real = ex._launch_forward
  ex._launch_forward = lambda *a, **kw: (seeds.append(ex._pinned_seed), real(*a, **kw))[1]
  try:
    torch.manual_seed(11)
    losses = loss_fn(model, batch)
    torch.mean(losses).backward()
    state = torch.get_rng_state()
  finally:
    ex._launch_forward = real
    model.eval()
    model.zero_grad()
  lv, pmf = loss_fn._on_device(batch.device)
  torch.manual_seed(11)
  torch.multinomial(pmf, 4, replacement=True)
  torch.randn_like(batch)
  want = int(torch.randint(0, 2 ** 62, (1,)).item())
  assert torch.equal(torch.get_rng_state(), state), 'the loss drew something else from the host generator'
  assert seeds == [want, want], (seeds, want)
  assert ex._pinned_seed is None and bool(torch.isfinite(losses).all())


# ---- the training step ------------------------------------------------------------------------------------------------------
def _run_steps(st, cfg, sde, model, steps=3, classes=None):
  state = make_state(st, cfg, model)
  seen = []
  real = st.losses.ConsistencyLoss.__call__

  def spy(self, *a, **kw):
    seen.append(self.N)
    return real(self, *a, **kw)

  st.losses.ConsistencyLoss.__call__ = spy
  try:
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    before = [p.detach().clone() for p in model.parameters()]
    for i in range(steps):
      batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(100 + i)).to(cfg.device)
      torch.manual_seed(50 + i)
      losses = step_fn(state, batch, *(() if classes is None else (classes,)))
      assert losses.shape == (4,) and bool(torch.isfinite(losses).all()) and bool((losses >= 0).all()), losses
      assert state['step'] == i + 1
  finally:
    st.losses.ConsistencyLoss.__call__ = real
    model.eval()
  assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters())), 'no parameter changed'
  return seen


def _step_cfg(st, family, **kw):
  base = st.configs.consistency(tiny_config(st, family), s0=2, s1=8)
  base.training.n_iters = 8
  base.optim.warmup = 2
  for k, v in kw.items():
    setattr(base.training, k, v)
  return base


def test_three_steps_follow_the_curriculum(st, hip_lib):
  cfg, sde, model = _model(st, _step_cfg(st, 'vp'), hip_lib)
  assert _run_steps(st, cfg, sde, model) == [3, 3, 5]


def test_fp16_training_precision_runs(st, hip_lib):
  cfg, sde, model = _model(st, _step_cfg(st, 'wide', precision='fp16'), hip_lib)
  assert _run_steps(st, cfg, sde, model, steps=2) == [3, 3]


def test_class_conditional_step_runs(st, hip_lib):
  base = _step_cfg(st, 'vp')
  base.model.num_classes = 3
  cfg, sde, model = _model(st, base, hip_lib)
  assert _run_steps(st, cfg, sde, model, steps=2, classes=torch.tensor([0, 2, 1, 3])) == [3, 3]
  with pytest.raises(ValueError, match='classes'):
    st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))(make_state(st, cfg, model), torch.zeros(4, 3, 16, 16, device=cfg.device))


# ---- the sampler with the closed-form network ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gaussian_reference():
  """Per variant: the levels, the recorded draws, the float64 restatement's result and the same in numpy fp32.  Once."""
  g = R.GaussianData((2, 3, 8, 8))
  rng = np.random.RandomState(5)
  out = {}
  for name, lv, clip in (('one', (80.,), False), ('three', (80., 0.821, 0.05), False), ('three-clipped', (80., 0.821, 0.05), True)):
    z = [rng.standard_normal(g.mu.shape).astype(np.float32) for _ in lv]
    lo, hi = (-1., 1.) if clip else (-INF, INF)
    F_of = lambda xin, sigma: g.F(xin, sigma, E32)
    x64 = R.sample_loop(F_of, lv, z, S_DATA, S_MIN, lo, hi)
    x32 = R.sample_loop(F_of, lv, z, S_DATA, S_MIN, lo, hi, dtype=np.float32)
    out[name] = dict(gauss=g, levels=lv, clip=clip, z=z, x64=x64, x32=x32)
  return out


@pytest.mark.parametrize('variant', ['one', 'three', 'three-clipped'])
def test_sampler_with_a_closed_form_network(st, hip_lib, gaussian_reference, variant):
  ref = gaussian_reference[variant]
  g, lv = ref['gauss'], ref['levels']
  dev = torch.device('cuda:0')
  mu = torch.from_numpy(g.mu.astype(np.float32)).to(dev)
  c2 = torch.from_numpy((g.c ** 2).astype(np.float32)).to(dev)
  calls = []

  def model_fn(xin, c_noise):
    assert c_noise.shape == (2,) and c_noise.dtype == torch.float32 and c_noise.device == xin.device
    sigma = f32(lv[len(calls)])                       # the loop evaluates at exactly the given levels, in order
    assert bool((c_noise == f32(np.log(sigma) / 4.)).all()), (float(c_noise[0]), sigma)
    calls.append(sigma)
    c_in, c_skip, c_out, _ = (f32(v) for v in R.boundary(sigma, S_DATA, E32))
    x = xin / c_in
    flow = mu + torch.sqrt((c2 + f32(E32) * f32(E32)) / (c2 + sigma * sigma)) * (x - mu)
    return (flow - c_skip * x) / c_out

  sch = st.consistency.consistency_schedule(st.sde_lib.EDM(S_MIN, S_MAX, S_DATA), lv, clip=ref['clip'])
  noise = iter(torch.from_numpy(e).to(dev) for e in ref['z'])
  count = []
  saved = hip_lib.ct_step_f32
  hip_lib.ct_step_f32 = lambda *a: (count.append(1), saved(*a))[1]
  try:
    x = torch.empty((2, 3, 8, 8), device=dev)
    out = st.consistency.consistency_sample(model_fn, sch, x, noise_fn=lambda v: next(noise))
  finally:
    hip_lib.ct_step_f32 = saved
  assert out is x, 'the state was not advanced in place'
  assert len(calls) == sch.nfe == len(lv) == len(count) and next(noise, None) is None
  got = out.cpu().double().numpy()
  own = R.rel(ref['x32'], ref['x64'])
  err = R.rel(got, ref['x64'])
  print(f'{variant}: product loop deviates {err:.2e} from the float64 restatement; the restatement in numpy fp32 deviates '
        f'{own:.2e}: tolerance {4 * own:.2e}')
  assert own > 0 and err <= 4 * own
  if ref['clip']:
    assert float(out.min()) >= -1. and float(out.max()) <= 1.
  if variant == 'one':
    exact = g.flow(80. * ref['z'][0].astype(np.float64), 80., E32)
    e_flow = R.rel(got, exact)
    print(f'one step against the exact flow: {e_flow:.2e}')
    assert e_flow <= 4 * own


# ---- the sampler on a tiny network -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', [(80.,), (80., 0.821)], ids=['one-step', 'two-step'])
def test_sampler_on_a_tiny_network(st, hip_lib, levels):
  cfg, sde, model = _tiny(st, hip_lib, 'vp')
  c = copy.deepcopy(cfg)
  c.sampling.ct_levels = levels
  shape = (2, c.data.num_channels, c.data.image_size, c.data.image_size)
  fn = st.sampling.get_sampling_fn(c, sde, shape, st.datasets.get_data_inverse_scaler(c), 1e-3)
  evals = []
  hook = model.module.register_forward_hook(lambda m, a, o: evals.append(1))
  try:
    torch.manual_seed(3)
    got, nfe = fn(model)
  finally:
    hook.remove()
  assert nfe == len(levels) == len(evals)
  assert got.shape == shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  assert float(got.min()) >= 0. and float(got.max()) <= 1., 'outside the clip range after the inverse scaler'
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again), 'two runs under one seed differ'
  torch.manual_seed(4)
  assert not torch.equal(got, fn(model)[0])
  c.sampling.precision = 'fp16'
  half, nfe = st.sampling.get_sampling_fn(c, sde, shape, st.datasets.get_data_inverse_scaler(c), 1e-3)(model)
  assert nfe == len(levels) and bool(torch.isfinite(half).all())


# ---- opt-in -------------------------------------------------------------------------------------------------------------------
def test_without_the_key_the_edm_loss_is_what_it_was(st, hip_lib, monkeypatch):
  """Under configs.edm (no training.consistency) the loss chosen is the EDM loss, and its losses for a seeded batch are
  bit-equal to those obtained with the new module out of reach: for the second evaluation the module is taken out of
  sys.modules and off the package (an import of it raises), which is what never having imported it amounts to for the code
  that runs."""
  cfg, sde, model = _model(st, st.configs.edm(tiny_config(st, 'vp')), hip_lib)
  model.eval()
  assert 'consistency' not in cfg.training
  batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(3)).to(cfg.device)

  def evaluate():
    loss_fn = st.losses._pick_loss_fn(cfg, sde, True)
    assert not hasattr(loss_fn, 'set_step') and 'get_edm_loss_fn' in loss_fn.__qualname__
    with patched_rng(17), torch.no_grad():
      return loss_fn(model, batch)

  with_module = evaluate()
  name = st.consistency.__name__
  monkeypatch.setitem(sys.modules, name, None)
  monkeypatch.delattr(st, 'consistency')
  with pytest.raises(ImportError):
    __import__(name)
  without = evaluate()
  direct = None
  with patched_rng(17), torch.no_grad():
    direct = st.losses.get_edm_loss_fn(cfg, sde, True)(model, batch)
  assert torch.equal(with_module, without) and torch.equal(with_module, direct) and bool(torch.isfinite(direct).all())
