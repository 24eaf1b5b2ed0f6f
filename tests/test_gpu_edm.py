"""The kernels of include/stk_edm.h (csrc/edm.hip), the fused EDM loss and the EDM sampler built on them, on the device.

The kernels against float64.  The bounds are the rounding model of the header's lines, not blanket tolerances: every output
element is an expression of rounded products, quotients and sums, and standard forward analysis bounds its error by gamma_k B,
where B is the same expression on absolute values and k the number of roundings on the longest path from an operand to the
result, gamma_k = k u / (1 - k u) < (k + 1) u, u = 2^-24.  The tests hold K = k + 1.  The scalars reach the reference as the
fp32 values the kernel receives.

  stk_edm_step_f32   D = cs xe + co F: (product, sum), k = 2 on B_D = |cs| |xe| + |co| |F|;  dn = (xe - D) / t: two more,
                     k = 4 on B_dn = (|xe| + B_D) / t;  slope = 0.5 d_prev + 0.5 dn: the halvings are exact, the sum is the
                     fifth, on B_s = 0.5 |d_prev| + 0.5 B_dn (the Euler stage has slope = dn: one rounding fewer, the bound
                     stays valid);  x_out = xb + h slope: k = 7 on B_x = |xb| + |h| B_s;  xin_out = c_next x_out: k = 8 on
                     |c_next| B_x.  K_D is not observable; K_DN = 5, K_X = 8, K_XIN = 9.
  stk_edm_churn_f32  x^ = x + c_eps eps: k = 2 on |x| + c_eps |eps|, K = 3;  xin = c_in_hat x^: k = 3, K = 4.
  stk_edm_loss_f32   x = y + sg n: 2;  c_skip x: 3;  + c_out F: 4;  - y: 5, on B_r = c_skip (|y| + sg |n|) + c_out |F| + |y|:
                     K_R = 6.  loss_out is compared with the float64 sum of the SAME fp32 squares (of the r the kernel wrote),
                     times lambda, over inner: the kernel's float64 sum of `inner` non-negative terms in any order differs by at
                     most inner 2^-53 relative, the product with lambda and the quotient add one 2^-53 each, and the result is
                     rounded to fp32 once: |loss - want| <= (2^-24 + (inner + 2) 2^-53) want, held with the factor 1 + 2^-20
                     that covers the second-order terms.
  stk_edm_loss_grad_f32  k = ((2 lambda) c_out) dloss (/ inner): the doubling is exact, two products and the quotient round
                     (inner <= 2^24 here, so its conversion does not), dF = k r is the fourth: K_G = 5 on |k| |r|.

Besides the bounds every output is compared BIT FOR BIT with a numpy float32 restatement of the header's lines (numpy rounds
each operation once and fuses nothing), and every in-place / NULL form the header allows with the separate-buffer form.

stk_edm_coeffs_f32: the five algebraic rows are float64 expressions of correctly rounded operations (product, sum, square
root, quotient) rounded to fp32 once, so numpy float64 in the same order reproduces them bit for bit; the logarithm of row 5
is not correctly rounded in either library, so c_noise is held to one fp32 unit in the last place.

The loop with a closed-form network, and the sampler on the tiny networks, against float64 loops: the tolerance is measured,
not fixed in advance -- the float64 reference loop is run again in fp32 (numpy for the closed-form network, torch for the tiny
networks: every operation rounded), and four times its deviation from float64 is what the product loop may deviate.  The
deviations are printed by the tests.  On the CPU the restatement in numpy fp32 deviates from float64 by 4.1e-7 relative at 18
steps without churn; the figures of the product loop on an MI355X are in MEASURED.
"""
import copy

import numpy as np
import pytest
import torch

import _edm_ref as R
from _model_util import Tap as _Tap, build_pair, patched_rng, tiny_config
from _stream_util import ROW_SHAPES, SHAPES, U, case_id, drawn_operands, nan as _nan, place, ptr as _ptr, stream as _stream, within

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file, worst case over the shapes, in units of u B against the bound held:
stk_edm_step_f32 x_out 3.78 (8), d_out 3.21 (5), xin_out 4.24 (9);  stk_edm_churn_f32 x_hat 1.92 (3), xin 2.47 (4);
stk_edm_loss_f32 r_out 3.03 (6), loss_out 1.00 of its bound (3000 rows of 4: a half-unit rounding to fp32 is the whole bound),
stk_edm_loss_grad_f32 dF 2.72 (5);  c_noise differs from numpy in 0 of 4097 levels.  Fused and torch-expression loss on the tiny
networks: losses 0.02 of their bound, the network-output gradient 0.38-0.45, both paths alike.  Closed-form loop, 18 steps:
the product loop deviates 3.7e-7 (deterministic) / 3.1e-7 (13 churned steps) from the float64 restatement, the numpy fp32
restatement 4.1e-7 / 3.3e-7.  Tiny networks, 6 steps: sampler 1.3e-6 (vp) / 1.6e-6 (ve) without churn, 1.7e-6 / 1.8e-6 with,
the torch fp32 loop 1.4e-6 / 1.6e-6 and 1.8e-6 / 1.8e-6.  fp16 against fp32 on the wide network after 11 evaluations: 3.9e-5."""

K_DN, K_X, K_XIN = 5, 8, 9
K_XHAT, K_CHURN_XIN = 3, 4
K_R, K_G = 6, 5
SIGMA_DATA = 0.5
EINVAL, EUNSUPPORTED = -1, -3
f32 = lambda v: float(np.float32(v))
# (cs, co, t, h, c_next): a step from t^ = 2.6 to 1.9 at sigma_data = 0.5
ROW = tuple(f32(v) for v in (0.0357, 0.491, 2.6, -0.7, 0.509))
@pytest.fixture(scope='module')
def operands():
  """Four fp32 tensors per shape on the host (numpy), drawn once: xb / y, xe / n, F, d_prev."""
  return drawn_operands()


# ---- stk_edm_step_f32 ---------------------------------------------------------------------------------------------------
def _step_restate(xb, xe, F, d_prev, row, dtype):
  """The header's lines in `dtype` -> (x_out, dn, xin, B_x, B_dn)."""
  cs, co, t, h, cn = (dtype(v) for v in row)
  xb, xe, F = xb.astype(dtype), xe.astype(dtype), F.astype(dtype)
  D = cs * xe + co * F
  dn = (xe - D) / t
  slope = dn if d_prev is None else dtype(0.5) * d_prev.astype(dtype) + dtype(0.5) * dn
  x_out = xb + h * slope
  b_D = abs(cs) * np.abs(xe) + abs(co) * np.abs(F)
  b_dn = (np.abs(xe) + b_D) / t
  b_s = b_dn if d_prev is None else 0.5 * np.abs(d_prev.astype(dtype)) + 0.5 * b_dn
  return x_out, dn, cn * x_out, np.abs(xb) + abs(h) * b_s, b_dn


def _step(lib, xb, xe, F, d_prev, row, x_out, d_out, xin_out):
  lib.edm_step_f32(xb.data_ptr(), xe.data_ptr(), F.data_ptr(), _ptr(d_prev), *row, x_out.data_ptr(), _ptr(d_out), _ptr(xin_out),
                   xb.numel(), _stream())


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_step_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  xb, xe, F, dp = operands[shape]
  worst = dict(x=0., d=0., xin=0.)
  for euler in (True, False):
    b, e, F_d, p_d = (place(t, dev, shifted) for t in (xb, xe, F, dp))
    h_xe, h_dp = (xb, None) if euler else (xe, dp)
    e_d = b if euler else e                               # the Euler stage: xe IS xb, the same pointer
    prev = None if euler else p_d
    want = _step_restate(xb, h_xe, F, h_dp, ROW, np.float64)
    bits = _step_restate(xb, h_xe, F, h_dp, ROW, np.float32)
    what = f'edm_step {shape} shifted={shifted} {"euler" if euler else "correction"}'
    x_out, d_out, xin_out = (_nan(shape, dev, shifted) for _ in range(3))
    _step(hip_lib, b, e_d, F_d, prev, ROW, x_out, d_out, xin_out)
    worst['x'] = max(worst['x'], within(x_out, want[0], want[3], K_X, what + ' x_out'))
    worst['d'] = max(worst['d'], within(d_out, want[1], want[4], K_DN, what + ' d_out'))
    worst['xin'] = max(worst['xin'], within(xin_out, want[2], abs(ROW[4]) * want[3], K_XIN, what + ' xin_out'))
    for got, ref, name in ((x_out, bits[0], 'x_out'), (d_out, bits[1], 'd_out'), (xin_out, bits[2], 'xin_out')):
      assert np.array_equal(got.cpu().numpy(), ref), f'{what}: {name} is not the fp32 restatement bit for bit'
    for t_d, t_h in ((b, xb), (e, xe), (F_d, F), (p_d, dp)):
      assert np.array_equal(t_d.cpu().numpy(), t_h), what + ': an operand was written'
    # every NULL combination of the optional outputs: the outputs that remain keep their bits
    for use_d, use_xin in ((True, False), (False, True), (False, False)):
      xo = _nan(shape, dev, shifted)
      do = _nan(shape, dev, shifted) if use_d else None
      xi = _nan(shape, dev, shifted) if use_xin else None
      _step(hip_lib, b, e_d, F_d, prev, ROW, xo, do, xi)
      assert torch.equal(xo, x_out) and (do is None or torch.equal(do, d_out)) and (xi is None or torch.equal(xi, xin_out)), what
    # in place: x_out = xb (and so = xe in the Euler stage), x_out = xe, d_out = d_prev
    ba, ea, pa = (place(t, dev, shifted) for t in (xb, xe, dp))
    xi = _nan(shape, dev, shifted)
    _step(hip_lib, ba, ba if euler else ea, F_d, None if euler else pa, ROW, ba, None if euler else pa, xi)
    assert torch.equal(ba, x_out) and torch.equal(xi, xin_out), what + ': x_out = xb differs from the separate-buffer form'
    if not euler:
      assert torch.equal(pa, d_out), what + ': d_out = d_prev differs from the separate-buffer form'
      ba, ea = place(xb, dev, shifted), place(xe, dev, shifted)
      _step(hip_lib, ba, ea, F_d, p_d, ROW, ea, None, None)
      assert torch.equal(ea, x_out), what + ': x_out = xe differs from the separate-buffer form'
      assert np.array_equal(ba.cpu().numpy(), xb)
  print(f'edm_step {shape} shifted={shifted}: worst x_out {worst["x"]:.2f} u B (bound {K_X}), d_out {worst["d"]:.2f} ({K_DN}), '
        f'xin_out {worst["xin"]:.2f} ({K_XIN})')


# ---- stk_edm_churn_f32 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_churn_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  x, eps = operands[shape][:2]
  c_eps, c_in = f32(1.37), f32(0.377)
  xd, ed = place(x, dev, shifted), place(eps, dev, shifted)
  xh, xin = _nan(shape, dev, shifted), _nan(shape, dev, shifted)
  call = lambda x_, e_, c, xh_, xin_: hip_lib.edm_churn_f32(x_.data_ptr(), _ptr(e_), c, c_in, _ptr(xh_), xin_.data_ptr(),
                                                             x_.numel(), _stream())
  call(xd, ed, c_eps, xh, xin)
  x64, e64 = x.astype(np.float64), eps.astype(np.float64)
  want = x64 + c_eps * e64
  mag = np.abs(x64) + c_eps * np.abs(e64)
  what = f'edm_churn {shape} shifted={shifted}'
  w1 = within(xh, want, mag, K_XHAT, what + ' x_hat')
  w2 = within(xin, c_in * want, c_in * mag, K_CHURN_XIN, what + ' xin')
  bits = x + np.float32(c_eps) * eps
  assert np.array_equal(xh.cpu().numpy(), bits) and np.array_equal(xin.cpu().numpy(), np.float32(c_in) * bits)
  assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(ed.cpu().numpy(), eps), 'an operand was written'
  # in place on the state
  xa, xi = place(x, dev, shifted), _nan(shape, dev, shifted)
  call(xa, ed, c_eps, xa, xi)
  assert torch.equal(xa, xh) and torch.equal(xi, xin)
  # no noise: x^ = x exactly, written or not
  xh0, xi0, xi1 = _nan(shape, dev, shifted), _nan(shape, dev, shifted), _nan(shape, dev, shifted)
  call(xd, None, 0., xh0, xi0)
  call(xd, None, 0., None, xi1)
  assert np.array_equal(xh0.cpu().numpy(), x) and np.array_equal(xi0.cpu().numpy(), np.float32(c_in) * x) and torch.equal(xi0, xi1)
  print(f'{what}: worst x_hat {w1:.2f} u B (bound {K_XHAT}), xin {w2:.2f} ({K_CHURN_XIN})')


# ---- stk_edm_coeffs_f32 -------------------------------------------------------------------------------------------------
def _coeffs(lib, sigma, dev):
  sg = torch.from_numpy(sigma).to(dev)
  coef = torch.full((6, sigma.shape[0]), float('nan'), device=dev)
  lib.edm_coeffs_f32(sg.data_ptr(), SIGMA_DATA, coef.data_ptr(), sigma.shape[0], _stream())
  return sg, coef


def test_coeffs_are_the_float64_expressions(hip_lib):
  dev = torch.device('cuda:0')
  sweep = np.exp(np.linspace(np.log(0.002), np.log(80.), 4093))
  sigma = np.concatenate([[0.002, 80.], sweep, [0.5, 1.0]]).astype(np.float32)
  _, coef = _coeffs(hip_lib, sigma, dev)
  got = coef.cpu().numpy()
  want = R.coeff_rows(sigma, SIGMA_DATA, np.float32)
  for k, name in enumerate(('c_in', 'c_in sigma', 'c_skip', 'c_out', 'lambda')):
    assert np.array_equal(got[k], want[k]), f'{name}: {int((got[k] != want[k]).sum())} of {sigma.size} differ from numpy float64'
  ulp = np.spacing(np.abs(want[5]))
  off = np.abs(got[5].astype(np.float64) - want[5].astype(np.float64)) / np.maximum(ulp, np.float32(1e-45))
  print(f'c_noise: {int((got[5] != want[5]).sum())} of {sigma.size} differ from numpy, worst {off.max():.1f} ulp')
  assert bool((off <= 1.).all())
  # against Table 1 as the paper writes it
  c_in, c_skip, c_out, c_noise, lam = R.table1(sigma.astype(np.float64), SIGMA_DATA)
  for k, ref in ((0, c_in), (2, c_skip), (3, c_out), (4, lam)):
    assert np.allclose(got[k], ref, rtol=2e-7, atol=0), k
  # a level the logarithm or the quotients cannot take yields NaN or inf in its column only
  _, bad = _coeffs(hip_lib, np.array([1., 0., -1., np.inf, np.nan, 2.], dtype=np.float32), dev)
  bad = bad.cpu().numpy()
  assert np.isfinite(bad[:, [0, 5]]).all() and not np.isfinite(bad[:, 1:5]).all(axis=0).any()


# ---- stk_edm_loss_f32 / stk_edm_loss_grad_f32 -----------------------------------------------------------------------------
def _levels(B):
  """B noise levels over the training range, the two ends included when there is room."""
  sg = np.exp(np.random.RandomState(B).uniform(np.log(0.02), np.log(20.), size=B))
  if B >= 2:
    sg[0], sg[-1] = 0.002, 80.
  return sg.astype(np.float32)


def _loss(lib, F, y, n, sg, coef, r_out, loss_out, reduce_mean, ws=None):
  B, inner = y.shape[0], y[0].numel()
  if ws is None:
    ws = torch.empty(int(lib.edm_ws_bytes(B, inner)), dtype=torch.uint8, device=y.device)
  lib.edm_loss_f32(F.data_ptr(), y.data_ptr(), n.data_ptr(), sg.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel(),
                   _ptr(r_out), loss_out.data_ptr(), B, inner, int(reduce_mean), _stream())


@pytest.mark.parametrize('shape,shifted', ROW_SHAPES, ids=case_id)
def test_loss_pair_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  y, n, F, _ = operands[shape]
  B, inner = shape[0], int(np.prod(shape[1:]))
  sigma = _levels(B)
  sg, coef = _coeffs(hip_lib, sigma, dev)
  rows = coef.cpu().numpy()
  w = lambda v, dt: v.astype(dt).reshape(B, 1, 1, 1)
  yd, nd, Fd = (place(t, dev, shifted) for t in (y, n, F))
  what = f'edm_loss {shape} shifted={shifted}'
  # r: float64 bound and fp32 bits
  y64, n64, F64 = (t.astype(np.float64) for t in (y, n, F))
  want_r = w(rows[2], np.float64) * (y64 + w(sigma, np.float64) * n64) + w(rows[3], np.float64) * F64 - y64
  mag_r = w(rows[2], np.float64) * (np.abs(y64) + w(sigma, np.float64) * np.abs(n64)) + w(rows[3], np.float64) * np.abs(F64) + np.abs(y64)
  bits_r = (w(rows[2], np.float32) * (y + w(sigma, np.float32) * n) + w(rows[3], np.float32) * F) - y
  assert bits_r.dtype == np.float32
  sq = (bits_r * bits_r).astype(np.float64).reshape(B, -1).sum(axis=1)          # the SAME fp32 squares, summed in float64
  go = np.random.RandomState(3).standard_normal(B).astype(np.float32)
  go_d = torch.from_numpy(go).to(dev)
  for reduce_mean in (False, True):
    r_out, loss_out = _nan(shape, dev, shifted), torch.full((B,), float('nan'), device=dev)
    _loss(hip_lib, Fd, yd, nd, sg, coef, r_out, loss_out, reduce_mean)
    w_r = within(r_out, want_r, mag_r, K_R, what + ' r_out')
    assert np.array_equal(r_out.cpu().numpy(), bits_r), what + ': r_out is not the fp32 restatement bit for bit'
    want_l = rows[4].astype(np.float64) * sq
    if reduce_mean:
      want_l = want_l / inner
    got_l = loss_out.cpu().double().numpy()
    assert np.isfinite(got_l).all()
    tol = (2. ** -24 + (inner + 2) * 2. ** -53) * (1 + 2. ** -20) * want_l
    worst_l = float((np.abs(got_l - want_l) / np.maximum(tol, 1e-300)).max())
    assert bool((np.abs(got_l - want_l) <= tol).all()), f'{what} reduce_mean={reduce_mean}: loss_out off by {worst_l:.2f} of its bound'
    # run to run, and without the residual: the same bits
    again, no_r = torch.full((B,), float('nan'), device=dev), torch.full((B,), float('nan'), device=dev)
    r_again = _nan(shape, dev, shifted)
    _loss(hip_lib, Fd, yd, nd, sg, coef, r_again, again, reduce_mean)
    _loss(hip_lib, Fd, yd, nd, sg, coef, None, no_r, reduce_mean)
    assert torch.equal(again, loss_out) and torch.equal(r_again, r_out) and torch.equal(no_r, loss_out), what + ': not reproducible'
    # the gradient on the residual the forward kept
    k32 = ((np.float32(2.) * rows[4]) * rows[3]) * go
    k64 = 2. * rows[4].astype(np.float64) * rows[3].astype(np.float64) * go.astype(np.float64)
    if reduce_mean:
      k32, k64 = k32 / np.float32(inner), k64 / inner
    dF = _nan(shape, dev, shifted)
    grad = lambda r_, out_: hip_lib.edm_loss_grad_f32(r_.data_ptr(), coef.data_ptr(), go_d.data_ptr(), out_.data_ptr(), B, inner,
                                                      int(reduce_mean), _stream())
    grad(r_out, dF)
    r64 = bits_r.astype(np.float64)
    w_g = within(dF, w(k64, np.float64) * r64, np.abs(w(k64, np.float64) * r64), K_G, what + ' dF')
    assert np.array_equal(dF.cpu().numpy(), w(k32, np.float32) * bits_r), what + ': dF is not the fp32 restatement bit for bit'
    assert np.array_equal(r_out.cpu().numpy(), bits_r), 'the residual was written'
    grad(r_out, r_out)                                   # in place
    assert torch.equal(r_out, dF), what + ': dF = r differs from the separate-buffer form'
    print(f'{what} reduce_mean={reduce_mean}: worst r_out {w_r:.2f} u B (bound {K_R}), loss_out {worst_l:.2f} of its bound, '
          f'dF {w_g:.2f} u B (bound {K_G})')
  for t_d, t_h in ((yd, y), (nd, n), (Fd, F)):
    assert np.array_equal(t_d.cpu().numpy(), t_h), what + ': an operand was written'


def test_perturb_gives_the_network_input(hip_lib, operands):
  """x_in = c_in y + (c_in sigma) n is stk_perturb_f32 of stk.h with a = row 0 and s = row 1 of the coefficients."""
  dev = torch.device('cuda:0')
  shape = (3, 3, 5, 7)
  y, n = operands[shape][:2]
  sigma = _levels(3)
  _, coef = _coeffs(hip_lib, sigma, dev)
  yd, nd, out = place(y, dev), place(n, dev), _nan(shape, dev, False)
  hip_lib.perturb_f32(yd.data_ptr(), nd.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(), out.data_ptr(), 3, 105, _stream())
  rows = coef.cpu().numpy()
  w = lambda v: v.reshape(3, 1, 1, 1)
  assert np.array_equal(out.cpu().numpy(), w(rows[0]) * y + w(rows[1]) * n)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(hip_lib):
  """Every refusal of the header returns before any launch: the outputs keep their sentinel."""
  dev = torch.device('cuda:0')
  B, shape = 2, (2, 3, 4, 4)
  inner, n = 48, 96
  a, b, c, d = (torch.randn(shape, device=dev) for _ in range(4))
  outs = [torch.full(shape, 7.0, device=dev) for _ in range(3)]
  sg = torch.tensor([0.5, 2.], device=dev)
  coef, loss, go = torch.full((6, B), 7.0, device=dev), torch.full((B,), 7.0, device=dev), torch.ones(B, device=dev)
  ws = torch.full((int(hip_lib.edm_ws_bytes(B, inner)) // 8 + 1,), 7.0, dtype=torch.float64, device=dev)
  ws_bytes = int(hip_lib.edm_ws_bytes(B, inner))
  assert ws_bytes == B * 8
  nan, inf = float('nan'), float('inf')
  s = _stream()

  def clean():
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [coef, loss, ws]), 'a refused call wrote'

  def step(xb=a, xe=a, F=b, d_prev=None, t=2.6, x_out=outs[0], d_out=outs[1], xin_out=outs[2], n=n):
    code = hip_lib.edm_step_f32.raw(_ptr(xb), _ptr(xe), _ptr(F), _ptr(d_prev), 0.04, 0.49, t, -0.7, 0.5, _ptr(x_out), _ptr(d_out),
                                    _ptr(xin_out), n, s)
    clean()
    return code

  assert step(xb=None) == EINVAL and step(xe=None) == EINVAL and step(F=None) == EINVAL and step(x_out=None) == EINVAL
  assert step(n=0) == EINVAL and step(n=-4) == EINVAL
  assert step(t=0.) == EINVAL and step(t=-1.) == EINVAL and step(t=nan) == EINVAL and step(t=inf) == EINVAL
  assert step(n=2 ** 31) == EUNSUPPORTED and step(n=2 ** 40) == EUNSUPPORTED

  def churn(x=a, eps=b, c_eps=1.5, x_hat=outs[0], xin=outs[1], n=n):
    code = hip_lib.edm_churn_f32.raw(_ptr(x), _ptr(eps), c_eps, 0.4, _ptr(x_hat), _ptr(xin), n, s)
    clean()
    return code

  assert churn(x=None) == EINVAL and churn(xin=None) == EINVAL and churn(x_hat=None) == EINVAL
  assert churn(eps=None, c_eps=1.5) == EINVAL and churn(c_eps=-1.) == EINVAL and churn(c_eps=nan) == EINVAL
  assert churn(n=0) == EINVAL and churn(n=2 ** 31) == EUNSUPPORTED

  def coeffs(sigma=sg, s_data=0.5, out=coef, B=B):
    code = hip_lib.edm_coeffs_f32.raw(_ptr(sigma), s_data, _ptr(out), B, s)
    clean()
    return code

  assert coeffs(sigma=None) == EINVAL and coeffs(out=None) == EINVAL and coeffs(B=0) == EINVAL and coeffs(B=-1) == EINVAL
  assert coeffs(s_data=0.) == EINVAL and coeffs(s_data=-0.5) == EINVAL and coeffs(s_data=nan) == EINVAL and coeffs(s_data=inf) == EINVAL
  good = torch.empty((6, B), device=dev)
  hip_lib.edm_coeffs_f32(sg.data_ptr(), 0.5, good.data_ptr(), B, s)

  def lossf(F=a, y=b, n_=c, sigma=sg, cf=good, w=ws, wb=ws_bytes, r=outs[0], out=loss, B=B, inner=inner):
    code = hip_lib.edm_loss_f32.raw(_ptr(F), _ptr(y), _ptr(n_), _ptr(sigma), _ptr(cf), _ptr(w), wb, _ptr(r), _ptr(out), B, inner, 0, s)
    clean()
    return code

  for key in ('F', 'y', 'n_', 'sigma', 'cf', 'w', 'out'):
    assert lossf(**{key: None}) == EINVAL, key
  assert lossf(B=0) == EINVAL and lossf(inner=0) == EINVAL and lossf(wb=ws_bytes - 1) == EINVAL
  misaligned = hip_lib.edm_loss_f32.raw(a.data_ptr(), b.data_ptr(), c.data_ptr(), sg.data_ptr(), good.data_ptr(), ws.data_ptr() + 4,
                                        ws_bytes, outs[0].data_ptr(), loss.data_ptr(), B, inner, 0, s)
  clean()
  assert misaligned == EINVAL
  assert lossf(B=2, inner=2 ** 30) == EUNSUPPORTED and lossf(B=1, inner=2 ** 31) == EUNSUPPORTED

  def gradf(r=a, cf=good, dl=go, out=outs[0], B=B, inner=inner):
    code = hip_lib.edm_loss_grad_f32.raw(_ptr(r), _ptr(cf), _ptr(dl), _ptr(out), B, inner, 1, s)
    clean()
    return code

  for key in ('r', 'cf', 'dl', 'out'):
    assert gradf(**{key: None}) == EINVAL, key
  assert gradf(B=0) == EINVAL and gradf(inner=-1) == EINVAL and gradf(B=2, inner=2 ** 30) == EUNSUPPORTED
  # ... and the accepted edge forms run
  assert step(x_out=torch.empty_like(a), d_out=None, xin_out=None) == 0
  assert churn(eps=None, c_eps=0., x_hat=None, xin=torch.empty_like(a)) == 0
  # the checked binding raises the package's error
  with pytest.raises(RuntimeError, match='stk_edm_step_f32 failed'):
    hip_lib.edm_step_f32(a.data_ptr(), a.data_ptr(), b.data_ptr(), None, 0.04, 0.49, 0., -0.7, 0.5, outs[0].data_ptr(), None, None, n, s)


# ---- the fused loss against the torch-expression loss ---------------------------------------------------------------------
_built = {}


def _tiny(st, lib, family):
  """(cfg, sde, model) of a tiny network under configs.edm, in eval mode: built once per family."""
  if family not in _built:
    cfg, _, sde, model, _ = build_pair(st, st.configs.edm(tiny_config(st, family)), lib)
    model.eval()
    _built[family] = (cfg, sde, model)
  return _built[family]


@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_fused_loss_matches_the_torch_expressions(st, hip_lib, family, reduce_mean):
  """Same seeds: sigma and n are equal (one CPU stream serves both), so the network inputs are; each path's losses and
  network-output gradient lie within the kernel bounds of the float64 restatement on ITS OWN network output."""
  cfg, sde, model = _tiny(st, hip_lib, family)
  cfg = copy.deepcopy(cfg)
  cfg.training.reduce_mean = reduce_mean
  dev = cfg.device
  B = 6
  batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(3)).to(dev)
  inner = batch[0].numel()
  loss_fn = st.losses.get_edm_loss_fn(cfg, sde, True)
  go = torch.randn(B, generator=torch.Generator().manual_seed(4)).to(dev)
  with patched_rng(17):
    sigma = torch.exp(-1.2 + 1.2 * torch.randn(B)).numpy()
    n = torch.randn_like(batch).cpu().numpy()
  rows = R.coeff_rows(sigma, SIGMA_DATA, np.float32).astype(np.float64)
  y = batch.cpu().numpy().astype(np.float64)
  w = lambda v: v.reshape(B, 1, 1, 1)
  sg64, n64 = sigma.astype(np.float64), n.astype(np.float64)
  calls = []
  saved_fused, saved_entry = st.losses.FUSED_LOSS, hip_lib.edm_loss_f32
  hip_lib.edm_loss_f32 = lambda *a: (calls.append('loss'), saved_entry(*a))[1]
  seen = {}
  try:
    for fused in (True, False):
      st.losses.FUSED_LOSS = fused
      tap = _Tap(model)
      model.zero_grad()
      with patched_rng(17):
        losses = loss_fn(tap, batch)
      (losses * go).sum().backward()
      assert calls == ['loss'], f'fused={fused}: stk_edm_loss_f32 ran {len(calls)} times so far'
      x_in, cond, F, _ = tap.seen[0]
      seen[fused] = (x_in, cond)
      F64 = F.detach().cpu().double().numpy()
      r = w(rows[2]) * (y + w(sg64) * n64) + w(rows[3]) * F64 - y
      mag = w(rows[2]) * (np.abs(y) + w(sg64) * np.abs(n64)) + w(rows[3]) * np.abs(F64) + np.abs(y)
      dr = K_R * U * mag
      scale = 1. / inner if reduce_mean else 1.
      want = rows[4] * (r * r).reshape(B, -1).sum(axis=1) * scale
      slack = rows[4] * (2 * np.abs(r) * dr + dr * dr).reshape(B, -1).sum(axis=1) * scale
      tol = slack + (2. ** -23 + (inner + 2) * 2. ** -53) * want
      got = losses.detach().cpu().double().numpy()
      worst = float((np.abs(got - want) / tol).max())
      k = 2. * rows[4] * rows[3] * go.cpu().double().numpy() * scale
      g_tol = np.abs(w(k)) * (dr + K_G * U * (np.abs(r) + dr))
      g_err = np.abs(F.grad.cpu().double().numpy() - w(k) * r)
      print(f'{family} reduce_mean={reduce_mean} fused={fused}: loss {worst:.3f} of its bound, dLoss/dF {float((g_err / g_tol).max()):.3f} of its bound')
      assert bool((np.abs(got - want) <= tol).all()) and bool((g_err <= g_tol).all())
  finally:
    st.losses.FUSED_LOSS, hip_lib.edm_loss_f32 = saved_fused, saved_entry
  # the network inputs of the two paths: x_in to the rounding of c_in y + (c_in sigma) n, c_noise to one unit in the last place
  x_want = w(rows[0]) * y + w(rows[1]) * n64
  x_mag = w(rows[0]) * np.abs(y) + w(rows[1]) * np.abs(n64)
  for fused in (True, False):
    within(seen[fused][0], x_want, x_mag, 4, f'{family} fused={fused} x_in')
  want_cond = np.exp(rows[5]) if cfg.model.embedding_type == 'fourier' else rows[5]
  for fused in (True, False):
    assert np.allclose(seen[fused][1].cpu().double().numpy(), want_cond, rtol=4 * U, atol=4e-8)


# ---- the loop with a closed-form network ----------------------------------------------------------------------------------
CHURN = dict(s_churn=40., s_tmin=0.05, s_tmax=50., s_noise=1.003)


@pytest.fixture(scope='module')
def gaussian_reference(st):
  """Per variant: the schedule, the start state (fp32), the recorded noise, the float64 restatement's result and the same
  in numpy fp32.  Computed once."""
  g = R.GaussianData((4, 3, 8, 8))
  x_T = g.prior(80.).astype(np.float32)
  sde = st.sde_lib.EDM()
  F_of = lambda xin, sigma: R.gaussian_F(g, xin, sigma)
  out = {}
  for name, opts in (('deterministic', {}), ('stochastic', CHURN)):
    sch = st.edm.edm_schedule(sde, 18, **opts)
    rng = np.random.RandomState(5)
    noise = [rng.standard_normal(x_T.shape).astype(np.float32) for _ in range(int((sch.gamma > 0).sum()))]
    x64 = R.launch_loop(sch, F_of, x_T, noise=noise)
    x32 = R.launch_loop(sch, F_of, x_T, noise=noise, dtype=np.float32)
    out[name] = dict(gauss=g, x_T=x_T, sch=sch, noise=noise, x64=x64, x32=x32)
  return out


class _Counted:
  """Counts the launches of the two sampler entries on a library for the length of a `with`."""

  def __init__(self, lib):
    self.lib, self.n = lib, dict(churn=0, step=0)

  def __enter__(self):
    self.saved = (self.lib.edm_churn_f32, self.lib.edm_step_f32)
    self.lib.edm_churn_f32 = lambda *a: (self.n.__setitem__('churn', self.n['churn'] + 1), self.saved[0](*a))[1]
    self.lib.edm_step_f32 = lambda *a: (self.n.__setitem__('step', self.n['step'] + 1), self.saved[1](*a))[1]
    return self.n

  def __exit__(self, *exc):
    self.lib.edm_churn_f32, self.lib.edm_step_f32 = self.saved
    return False


@pytest.mark.parametrize('variant', ['deterministic', 'stochastic'])
def test_loop_with_a_closed_form_network(st, hip_lib, gaussian_reference, variant):
  ref = gaussian_reference[variant]
  sch, g = ref['sch'], ref['gauss']
  dev = torch.device('cuda:0')
  mu = torch.from_numpy(g.mu.astype(np.float32)).to(dev)
  c2 = torch.from_numpy((g.c ** 2).astype(np.float32)).to(dev)
  levels = [float(t) for pair in zip(sch.euler[:, 2], list(sch.correct[:, 2]) + [0.]) for t in pair][:sch.nfe]
  calls = []

  def model_fn(xin, c_noise):
    assert c_noise.shape == (4,) and c_noise.dtype == torch.float32 and c_noise.device == xin.device
    sigma = levels[len(calls)]                         # the loop evaluates at exactly the schedule's levels, in order
    assert bool((c_noise == f32(np.log(sigma) / 4.)).all()), (float(c_noise[0]), sigma)
    calls.append(sigma)
    c_in, c_skip, c_out, _, _ = (f32(v) for v in R.table1(sigma, SIGMA_DATA))
    x = xin / c_in
    D = mu + c2 / (c2 + f32(sigma) * f32(sigma)) * (x - mu)
    return (D - c_skip * x) / c_out

  noise = iter(torch.from_numpy(e).to(dev) for e in ref['noise'])
  x = torch.from_numpy(ref['x_T']).to(dev)
  with _Counted(hip_lib) as count:
    out = st.edm.edm_sample(model_fn, sch, x, noise_fn=lambda v: next(noise))
  assert out is x, 'the state was not advanced in place'
  churned = int((sch.gamma > 0).sum())
  assert len(calls) == sch.nfe == 35 and count['step'] == 35 and count['churn'] == (1 if variant == 'deterministic' else churned + (sch.gamma[0] == 0))
  assert count['step'] + count['churn'] == sch.launches
  assert next(noise, None) is None, 'not every recorded eps was drawn'
  got = out.cpu().double().numpy()
  own = R.rel(ref['x32'], ref['x64'])
  err = R.rel(got, ref['x64'])
  print(f'{variant}: product loop deviates {err:.2e} from the float64 restatement; the restatement in numpy fp32 deviates '
        f'{own:.2e}: tolerance {4 * own:.2e}; error against the exact flow {R.rel(got, g.flow(ref["x_T"].astype(np.float64), 80., 0.)):.3e}')
  assert err <= 4 * own


# ---- the sampler on the tiny networks ---------------------------------------------------------------------------------------
STEPS = 6


def _shape(cfg):
  return (2, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)


def _sampler(st, cfg, sde, **options):
  c = copy.deepcopy(cfg)
  c.sampling.edm_steps = STEPS
  for k, v in options.items():
    setattr(c.sampling, k, v)
  return st.sampling.get_sampling_fn(c, sde, _shape(c), st.datasets.get_data_inverse_scaler(c), 1e-3)


def _by_hand(st, cfg, sde, model, dtype, seed, **opts):
  """The test's own loop: the same engine network, the updates in torch `dtype` from the schedule's rows."""
  sch = st.edm.edm_schedule(sde, STEPS, **opts)
  F_fn = st.models.utils.get_edm_model_fn(cfg, model, train=False)
  c = (lambda v: float(v)) if dtype == torch.float64 else f32
  torch.manual_seed(seed)
  with torch.no_grad():
    x = sde.prior_sampling(_shape(cfg)).to(cfg.device).to(dtype)
    ones = torch.ones(x.shape[0], device=x.device)
    net = lambda xin, row: F_fn(xin.float().contiguous(), ones * f32(row[5])).to(dtype)
    xin = None
    for i in range(sch.steps):
      if sch.gamma[i] > 0.:
        x = x + c(sch.c_eps[i]) * torch.randn_like(x.float()).to(dtype)
        xin = c(sch.c_in_hat[i]) * x
      elif i == 0:
        xin = c(sch.c_in_hat[0]) * x
      cs, co, t, h, cn = (c(v) for v in sch.euler[i][:5])
      d = (x - (cs * x + co * net(xin, sch.euler[i]))) / t
      x1 = x + h * d
      xin = cn * x1
      if i == sch.steps - 1:
        x = x1
        break
      cs, co, t, h, cn = (c(v) for v in sch.correct[i][:5])
      dn = (x1 - (cs * x1 + co * net(xin, sch.correct[i]))) / t
      x = x + h * (0.5 * d + 0.5 * dn)
      xin = cn * x
    return st.datasets.get_data_inverse_scaler(cfg)(x)


def _rel(a, b):
  return R.rel(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy())


@pytest.mark.parametrize('churned', [False, True], ids=['deterministic', 'stochastic'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_sampler_matches_a_float64_loop(st, hip_lib, family, churned):
  cfg, sde, model = _tiny(st, hip_lib, family)
  opts = dict(s_churn=12., s_tmin=0.05, s_tmax=50., s_noise=1.003) if churned else {}
  fn = _sampler(st, cfg, sde, **{'edm_' + k: v for k, v in opts.items()})
  sch = st.edm.edm_schedule(sde, STEPS, **opts)
  assert bool((sch.gamma > 0).any()) == churned
  evals = []
  hook = model.module.register_forward_hook(lambda m, a, o: evals.append(1))
  try:
    torch.manual_seed(3)
    with _Counted(hip_lib) as count:
      got, nfe = fn(model)
  finally:
    hook.remove()
  assert nfe == 2 * STEPS - 1 == len(evals) and count['step'] == 2 * STEPS - 1
  assert count['step'] + count['churn'] == sch.launches
  assert got.shape == _shape(cfg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again), 'two runs under one seed differ'
  want = _by_hand(st, cfg, sde, model, torch.float64, 3, **opts)
  own = _rel(_by_hand(st, cfg, sde, model, torch.float32, 3, **opts), want)
  err = _rel(got, want)
  print(f'{family} churned={churned}: sampler deviates {err:.2e} from the float64 loop; the same loop in torch fp32 deviates '
        f'{own:.2e}: tolerance {4 * own:.2e}')
  assert err <= 4 * own


def test_the_only_draw_is_the_prior(st, hip_lib):
  """With s_churn = 0 the generators after a whole run are where one sde.prior_sampling(shape) alone leaves them."""
  cfg, sde, model = _tiny(st, hip_lib, 'vp')
  fn = _sampler(st, cfg, sde)
  torch.manual_seed(5)
  fn(model)
  after_run = (torch.get_rng_state(), torch.cuda.get_rng_state())
  torch.manual_seed(5)
  sde.prior_sampling(_shape(cfg))
  after_prior = (torch.get_rng_state(), torch.cuda.get_rng_state())
  torch.manual_seed(5)
  untouched = (torch.get_rng_state(), torch.cuda.get_rng_state())
  assert torch.equal(after_run[0], after_prior[0]) and torch.equal(after_run[1], after_prior[1])
  assert not (torch.equal(after_prior[0], untouched[0]) and torch.equal(after_prior[1], untouched[1])), 'the prior drew nothing'


def test_fp16_runs(st, hip_lib):
  """precision = 'fp16' (the network only): finite samples, the same counts.  No threshold on the difference from fp32: sample
  quality in that mode is unmeasured everywhere in this project.  Only the wide network has layers that take the fp16 forms."""
  cfg, sde, model = _tiny(st, hip_lib, 'wide')
  outs = {}
  for precision in ('fp32', 'fp16'):
    torch.manual_seed(9)
    with _Counted(hip_lib) as count:
      outs[precision], nfe = _sampler(st, cfg, sde, precision=precision)(model)
    assert nfe == 2 * STEPS - 1 and count['step'] == nfe and count['churn'] == 1 and bool(torch.isfinite(outs[precision]).all())
  diff = float((outs['fp16'] - outs['fp32']).abs().max())
  print(f'wide: fp16 against fp32 after {nfe} evaluations: max |difference| {diff:.3e}')
  assert diff > 0, 'the fp16 mode did not reach the network'
