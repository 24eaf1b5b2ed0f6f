"""The kernels of include/stk_flow.h (csrc/flow.hip), the fused rectified-flow loss and the flow sampler built on them, on
the device.

The kernels against float64.  As in tests/test_gpu_edm.py the bounds are the rounding model of the header's lines, not blanket
tolerances: every output element is an expression of rounded products and sums, and forward analysis bounds its error by
gamma_k B, where B is the same expression on absolute values and k the number of roundings on the longest path from an
operand to the result, gamma_k = k u / (1 - k u) < (k + 1) u, u = 2^-24.  The tests hold K = k + 1.  The scalars reach the
reference as the fp32 values the kernel receives.

  stk_flow_step_f32  Euler: m = cx xb and p = cv v round once each, x = m + p is the second on either path: k = 2 on
                     B = |cx| |xb| + |cv| |v|, K_EULER = 3.  Correction: slope = 0.5 v_prev + 0.5 v has exact halvings and one
                     rounded sum, p = cv slope is the second, x = m + p the third: k = 3 on |cx| |xb| + |cv| (0.5 |v_prev| +
                     0.5 |v|), K_HEUN = 4.  Stochastic: m + p as in Euler (2), cn eps rounds once, the last sum is the third on
                     the longer path: k = 3 on |cx| |xb| + |cv| |v| + cn |eps|, K_NOISE = 4.
  stk_flow_loss_f32  u = n - y: 1;  r = F - u: 2, on B_r = |F| + |n| + |y|: K_R = 3.  loss_out is compared with the float64 sum
                     of the SAME fp32 squares (of the r the kernel wrote), over inner under reduce_mean: the bound
                     tests/test_gpu_edm.py derives for stk_edm_loss_f32 with its lambda-product removed -- the kernel's float64
                     sum of `inner` non-negative terms in any order differs by at most inner 2^-53 relative, the quotient adds
                     one 2^-53, and the result is rounded to fp32 once: |loss - want| <= (2^-24 + (inner + 1) 2^-53) want, held
                     with the factor 1 + 2^-20 that covers the second-order terms.
  stk_flow_loss_grad_f32  k = 2 dloss is exact, k / (float)inner rounds once (inner <= 2^24 here, so its conversion does not),
                     dF = k r is the second: K_G = 3 on |k| |r|.

Besides the bounds every output is compared BIT FOR BIT with the numpy float32 restatement of tests/_flow_ref.py (numpy rounds
each operation once and fuses nothing), and every in-place / NULL form the header allows with the separate-buffer form.  The
outputs of the step start as NaN inside guarded buffers: nothing is left unwritten, nothing is written outside.

The loops against float64 loops: the tolerance is measured, not fixed in advance -- the float64 reference loop is run again in
fp32 (numpy for the closed-form velocity, torch for the tiny networks: every operation rounded), and four times its deviation
from float64 is what the product loop may deviate.  The deviations are printed by the tests; the figures of one run on an
MI355X are in MEASURED.
"""
import copy

import numpy as np
import pytest
import torch

import _flow_ref as R
from _model_util import Tap as _Tap, build_pair, patched_rng, tiny_config
from _stream_util import ROW_SHAPES, SHAPES, U, Guarded, case_id, drawn_operands, nan as _nan, place, ptr as _ptr, stream as _stream, within

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file, worst case over the shapes, in units of u B against the bound held:
stk_flow_step_f32 Euler 1.83 (3), correction 2.19 (4), stochastic 2.74 (4);  stk_flow_loss_f32 r_out 1.96 (3), loss_out 0.99 of
its bound (3000 rows of 4: a half-unit rounding to fp32 is the whole bound), stk_flow_loss_grad_f32 dF 1.65 (3).  Fused and
torch-expression loss on the tiny networks: losses 0.06-0.10 of their bound, the network-output gradient 0.41-0.51, both paths
alike.  Closed-form Gaussian loop, 50 steps at shift 3: the product loop deviates 2.15e-7 (order 1) / 3.10e-7 (order 2) /
4.15e-7 (eta = 0.7, 49 draws) from the float64 restatement, the numpy fp32 restatement the same 2.15e-7 / 3.10e-7 / 4.15e-7;
order 2 misses the exact map x(0) = c x(1) by 1.333e-3, which is what the variance recursion allows.  Tiny networks, 6 steps:
sampler 7.5e-8 / 9.9e-8 / 1.4e-7 (positional: order 1 / order 2 / shift 3 with eta 0.7) and 1.1e-7 / 1.4e-7 / 2.1e-7 (fourier),
the torch fp32 loop the same figures; under guidance 1.5 8.5e-8 beside 8.5e-8.  rk45 on N(0, c^2): c = 0.5 44 evaluations on
the device and in float64 on the CPU, deviating 3.5e-7 where the CPU solver on the fp32 field deviates 3.1e-7; c = 2 38 and
38, 5.30e-6 beside 5.27e-6.  fp16 against fp32 on the wide network after 11 evaluations: 2.39e-5, the EDM sampler's own pair on the same
network, measured in the same test: 3.89e-5."""

K_EULER, K_HEUN, K_NOISE = 3, 4, 4
K_R, K_G = 3, 3
EINVAL, EUNSUPPORTED = -1, -3
f32 = lambda v: float(np.float32(v))
# (cx, cv, cn) of a stochastic step from t = 0.62 by D = 0.04 at eta = 0.7, and of the deterministic step of the same length
ROW_NOISE = tuple(f32(v) for v in (1. - 0.7 * 0.04, -0.04 * (1. + 0.7 * 0.38), np.sqrt(2. * 0.7 * 0.62 * 0.04)))
ROW_ODE = (1., f32(-0.04), 0.)
PLACEMENT = {False: 'aligned', True: 'entered-one-in'}


@pytest.fixture(scope='module')
def operands():
  """Four fp32 tensors per shape on the host (numpy), drawn once: xb / y, v / n, v_prev / F, eps."""
  return drawn_operands()


# ---- stk_flow_step_f32 --------------------------------------------------------------------------------------------------
def _step(lib, xb, v, v_prev, eps, row, x_out):
  lib.flow_step_f32(xb.data_ptr(), v.data_ptr(), _ptr(v_prev), _ptr(eps), *row, x_out.data_ptr(), xb.numel(), _stream())


FORMS = (('euler', ROW_ODE, False, False, K_EULER), ('correction', ROW_ODE, True, False, K_HEUN),
         ('stochastic', ROW_NOISE, False, True, K_NOISE))


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_step_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  xb, v, vp, eps = operands[shape]
  b, v_d, p_d, e_d = (place(t, dev, shifted) for t in (xb, v, vp, eps))
  nans = np.full(shape, np.nan, dtype=np.float32)
  worst = {}
  for name, row, use_prev, use_eps, K in FORMS:
    h_prev, h_eps = (vp if use_prev else None), (eps if use_eps else None)
    d_prev, d_eps = (p_d if use_prev else None), (e_d if use_eps else None)
    want, mag = R.step(xb, v, h_prev, h_eps, row, np.float64)
    bits, _ = R.step(xb, v, h_prev, h_eps, row, np.float32)
    assert bits.dtype == np.float32
    what = f'flow_step {shape} shifted={shifted} {name}'
    out = Guarded(nans, dev, PLACEMENT[shifted])
    _step(hip_lib, b, v_d, d_prev, d_eps, row, out.view)
    out.check(what)
    worst[name] = within(out.view, want, mag, K, what)
    assert np.array_equal(out.view.cpu().numpy(), bits), f'{what}: x_out is not the fp32 restatement bit for bit'
    if row[0] == 1.:
      slope = v if h_prev is None else np.float32(0.5) * vp + np.float32(0.5) * v
      assert np.array_equal(bits, xb + np.float32(row[1]) * slope), 'cx = 1 is not an exact product'
    # in place: x_out = xb
    state = Guarded(xb, dev, PLACEMENT[shifted])
    _step(hip_lib, state.view, v_d, d_prev, d_eps, row, state.view)
    state.check(what + ' in place')
    assert torch.equal(state.view, out.view), what + ': x_out = xb differs from the separate-buffer form'
  for t_d, t_h in ((b, xb), (v_d, v), (p_d, vp), (e_d, eps)):
    assert np.array_equal(t_d.cpu().numpy(), t_h), f'flow_step {shape}: an operand was written'
  # eps given with cn = 0 adds an exact zero: the Euler bits
  out = Guarded(nans, dev, PLACEMENT[shifted])
  _step(hip_lib, b, v_d, None, e_d, ROW_ODE, out.view)
  assert np.array_equal(out.view.cpu().numpy(), R.step(xb, v, None, eps, ROW_ODE, np.float32)[0])
  print(f'flow_step {shape} shifted={shifted}: worst euler {worst["euler"]:.2f} u B (bound {K_EULER}), correction '
        f'{worst["correction"]:.2f} ({K_HEUN}), stochastic {worst["stochastic"]:.2f} ({K_NOISE})')


# ---- stk_flow_loss_f32 / stk_flow_loss_grad_f32 ---------------------------------------------------------------------------
def _loss(lib, F, y, n, r_out, loss_out, reduce_mean, ws=None):
  B, inner = y.shape[0], y[0].numel()
  if ws is None:
    ws = torch.empty(int(lib.flow_ws_bytes(B, inner)), dtype=torch.uint8, device=y.device)
  lib.flow_loss_f32(F.data_ptr(), y.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), _ptr(r_out), loss_out.data_ptr(), B, inner,
                    int(reduce_mean), _stream())


@pytest.mark.parametrize('shape,shifted', ROW_SHAPES, ids=case_id)
def test_loss_pair_matches_float64_and_the_fp32_restatement(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  y, n, F, _ = operands[shape]
  B, inner = shape[0], int(np.prod(shape[1:]))
  w = lambda v, dt: v.astype(dt).reshape(B, 1, 1, 1)
  yd, nd, Fd = (place(t, dev, shifted) for t in (y, n, F))
  what = f'flow_loss {shape} shifted={shifted}'
  want_r, mag_r = R.residual(F, y, n, np.float64)
  bits_r, _ = R.residual(F, y, n, np.float32)
  assert bits_r.dtype == np.float32
  sq = (bits_r * bits_r).astype(np.float64).reshape(B, -1).sum(axis=1)          # the SAME fp32 squares, summed in float64
  go = np.random.RandomState(3).standard_normal(B).astype(np.float32)
  go_d = torch.from_numpy(go).to(dev)
  for reduce_mean in (False, True):
    r_out, loss_out = _nan(shape, dev, shifted), torch.full((B,), float('nan'), device=dev)
    _loss(hip_lib, Fd, yd, nd, r_out, loss_out, reduce_mean)
    w_r = within(r_out, want_r, mag_r, K_R, what + ' r_out')
    assert np.array_equal(r_out.cpu().numpy(), bits_r), what + ': r_out is not the fp32 restatement bit for bit'
    want_l = sq / inner if reduce_mean else sq
    got_l = loss_out.cpu().double().numpy()
    assert np.isfinite(got_l).all()
    tol = (2. ** -24 + (inner + 1) * 2. ** -53) * (1 + 2. ** -20) * want_l
    worst_l = float((np.abs(got_l - want_l) / np.maximum(tol, 1e-300)).max())
    assert bool((np.abs(got_l - want_l) <= tol).all()), f'{what} reduce_mean={reduce_mean}: loss_out off by {worst_l:.2f} of its bound'
    # run to run, and without the residual: the same bits
    again, no_r = torch.full((B,), float('nan'), device=dev), torch.full((B,), float('nan'), device=dev)
    r_again = _nan(shape, dev, shifted)
    _loss(hip_lib, Fd, yd, nd, r_again, again, reduce_mean)
    _loss(hip_lib, Fd, yd, nd, None, no_r, reduce_mean)
    assert torch.equal(again, loss_out) and torch.equal(r_again, r_out) and torch.equal(no_r, loss_out), what + ': not reproducible'
    # the gradient on the residual the forward kept
    k32 = np.float32(2.) * go
    k64 = 2. * go.astype(np.float64)
    if reduce_mean:
      k32, k64 = k32 / np.float32(inner), k64 / inner
    assert k32.dtype == np.float32
    dF = _nan(shape, dev, shifted)
    grad = lambda r_, out_: hip_lib.flow_loss_grad_f32(r_.data_ptr(), go_d.data_ptr(), out_.data_ptr(), B, inner, int(reduce_mean),
                                                       _stream())
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
  """x_t = a y + t n with a = 1 - t is stk_perturb_f32 of stk.h, bit for bit the fp32 expression."""
  dev = torch.device('cuda:0')
  shape = (3, 3, 5, 7)
  y, n = operands[shape][:2]
  t = np.array([2. ** -24, 0.37, 1.], dtype=np.float32)
  a = np.float32(1.) - t
  yd, nd, ad, td, out = place(y, dev), place(n, dev), place(a, dev), place(t, dev), _nan(shape, dev, False)
  hip_lib.perturb_f32(yd.data_ptr(), nd.data_ptr(), ad.data_ptr(), td.data_ptr(), out.data_ptr(), 3, 105, _stream())
  w = lambda v: v.reshape(3, 1, 1, 1)
  assert np.array_equal(out.cpu().numpy(), w(a) * y + w(t) * n)
  assert np.array_equal(out.cpu().numpy()[2], n[2]), 'at t = 1 the input is the noise'


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(hip_lib):
  """Every refusal of the header returns before any launch: the outputs keep their sentinel."""
  dev = torch.device('cuda:0')
  B, shape = 2, (2, 3, 4, 4)
  inner, n = 48, 96
  a, b, c, d = (torch.randn(shape, device=dev) for _ in range(4))
  outs = [torch.full(shape, 7.0, device=dev) for _ in range(2)]
  loss, go = torch.full((B,), 7.0, device=dev), torch.ones(B, device=dev)
  ws_bytes = int(hip_lib.flow_ws_bytes(B, inner))
  assert ws_bytes == B * 8
  ws = torch.full((ws_bytes // 8 + 1,), 7.0, dtype=torch.float64, device=dev)
  nan, inf = float('nan'), float('inf')
  s = _stream()

  def clean():
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [loss, ws]), 'a refused call wrote'

  def step(xb=a, v=b, v_prev=None, eps=None, cn=0., x_out=outs[0], n=n):
    code = hip_lib.flow_step_f32.raw(_ptr(xb), _ptr(v), _ptr(v_prev), _ptr(eps), 0.97, -0.05, cn, _ptr(x_out), n, s)
    clean()
    return code

  assert step(xb=None) == EINVAL and step(v=None) == EINVAL and step(x_out=None) == EINVAL
  assert step(n=0) == EINVAL and step(n=-4) == EINVAL
  assert step(eps=None, cn=0.2) == EINVAL, 'eps NULL with cn != 0'
  assert step(eps=c, cn=-0.2) == EINVAL and step(eps=c, cn=nan) == EINVAL and step(cn=nan) == EINVAL
  assert step(v_prev=c, eps=d, cn=0.2) == EINVAL and step(v_prev=c, eps=d, cn=0.) == EINVAL, 'v_prev and eps both given'
  assert step(n=2 ** 31) == EUNSUPPORTED and step(n=2 ** 40) == EUNSUPPORTED

  def lossf(F=a, y=b, n_=c, w=ws, wb=ws_bytes, r=outs[0], out=loss, B=B, inner=inner):
    code = hip_lib.flow_loss_f32.raw(_ptr(F), _ptr(y), _ptr(n_), _ptr(w), wb, _ptr(r), _ptr(out), B, inner, 0, s)
    clean()
    return code

  for key in ('F', 'y', 'n_', 'w', 'out'):
    assert lossf(**{key: None}) == EINVAL, key
  assert lossf(B=0) == EINVAL and lossf(B=-2) == EINVAL and lossf(inner=0) == EINVAL and lossf(wb=ws_bytes - 1) == EINVAL
  misaligned = hip_lib.flow_loss_f32.raw(a.data_ptr(), b.data_ptr(), c.data_ptr(), ws.data_ptr() + 4, ws_bytes, outs[0].data_ptr(),
                                         loss.data_ptr(), B, inner, 0, s)
  clean()
  assert misaligned == EINVAL
  assert lossf(B=2, inner=2 ** 30) == EUNSUPPORTED and lossf(B=1, inner=2 ** 31) == EUNSUPPORTED

  def gradf(r=a, dl=go, out=outs[0], B=B, inner=inner):
    code = hip_lib.flow_loss_grad_f32.raw(_ptr(r), _ptr(dl), _ptr(out), B, inner, 1, s)
    clean()
    return code

  for key in ('r', 'dl', 'out'):
    assert gradf(**{key: None}) == EINVAL, key
  assert gradf(B=0) == EINVAL and gradf(inner=-1) == EINVAL and gradf(B=2, inner=2 ** 30) == EUNSUPPORTED
  # ... and the accepted edge forms run: infinite cn is no refusal of the header, eps with cn = 0, r_out NULL
  assert step(x_out=torch.empty_like(a)) == 0 and step(eps=c, cn=0., x_out=torch.empty_like(a)) == 0
  assert step(v_prev=c, x_out=torch.empty_like(a)) == 0
  assert lossf(r=None, out=torch.empty_like(loss), w=torch.empty(ws_bytes, dtype=torch.uint8, device=dev)) == 0
  # the checked binding raises the package's error
  with pytest.raises(RuntimeError, match='stk_flow_step_f32 failed'):
    hip_lib.flow_step_f32(a.data_ptr(), b.data_ptr(), None, None, 1., -0.05, 0.3, outs[0].data_ptr(), n, s)
  clean()


# ---- the fused loss against the torch-expression loss ---------------------------------------------------------------------
_built = {}


def _tiny(st, lib, family, num_classes=0):
  """(cfg, sde, model) of a tiny network under configs.flow, in eval mode: built once per family."""
  key = (family, num_classes)
  if key not in _built:
    base = st.configs.flow(tiny_config(st, family))
    if num_classes:
      base.model.num_classes = num_classes
    cfg, _, sde, model, _ = build_pair(st, base, lib)
    model.eval()
    _built[key] = (cfg, sde, model)
  return _built[key]


@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('family', ['vp', 've'], ids=['positional', 'fourier'])
def test_fused_loss_matches_the_torch_expressions(st, hip_lib, family, reduce_mean):
  """Same seeds: t and n are equal (one CPU stream serves both paths, and both consume exactly the [B] draw and the
  randn_like), so the network inputs are; each path's losses and network-output gradient lie within the kernel bounds of the
  float64 restatement on ITS OWN network output."""
  cfg, sde, model = _tiny(st, hip_lib, family)
  cfg = copy.deepcopy(cfg)
  cfg.training.reduce_mean = reduce_mean
  assert cfg.model.embedding_type == ('fourier' if family == 've' else 'positional')
  dev = cfg.device
  B = 6
  batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(3)).to(dev)
  inner = batch[0].numel()
  loss_fn = st.losses.get_flow_loss_fn(cfg, sde, True)
  go = torch.randn(B, generator=torch.Generator().manual_seed(4)).to(dev)
  with patched_rng(17):
    t_dev = torch.sigmoid(0. + 1. * torch.randn(B, device=dev)).to(torch.float32)      # the loss's own expression, on its device
    n = torch.randn_like(batch).cpu().numpy()
    next_draw = torch.rand(3)
  t = t_dev.cpu().numpy()
  y = batch.cpu().numpy().astype(np.float64)
  n64 = n.astype(np.float64)
  w = lambda v: v.reshape(B, 1, 1, 1)
  calls = []
  saved_fused, saved_entry = st.losses.FUSED_LOSS, hip_lib.flow_loss_f32
  hip_lib.flow_loss_f32 = lambda *a: (calls.append('loss'), saved_entry(*a))[1]
  seen = {}
  try:
    for fused in (True, False):
      st.losses.FUSED_LOSS = fused
      tap = _Tap(model)
      model.zero_grad()
      with patched_rng(17):
        losses = loss_fn(tap, batch)
        assert torch.equal(torch.rand(3), next_draw), f'fused={fused}: the loss consumed other draws than randn(B), randn_like'
      (losses * go).sum().backward()
      assert calls == ['loss'], f'fused={fused}: stk_flow_loss_f32 ran {len(calls)} times so far'
      x_in, cond, F, _ = tap.seen[0]
      seen[fused] = (x_in, cond)
      F64 = F.detach().cpu().double().numpy()
      r, mag = R.residual(F64, y, n64, np.float64)
      dr = K_R * U * mag
      scale = 1. / inner if reduce_mean else 1.
      want = (r * r).reshape(B, -1).sum(axis=1) * scale
      slack = (2 * np.abs(r) * dr + dr * dr).reshape(B, -1).sum(axis=1) * scale
      tol = slack + (2. ** -23 + (inner + 1) * 2. ** -53) * want
      got = losses.detach().cpu().double().numpy()
      worst = float((np.abs(got - want) / tol).max())
      k = 2. * go.cpu().double().numpy() * scale
      g_tol = np.abs(w(k)) * (dr + K_G * U * (np.abs(r) + dr))
      g_err = np.abs(F.grad.cpu().double().numpy() - w(k) * r)
      print(f'{family} reduce_mean={reduce_mean} fused={fused}: loss {worst:.3f} of its bound, dLoss/dF {float((g_err / g_tol).max()):.3f} of its bound')
      assert bool((np.abs(got - want) <= tol).all()) and bool((g_err <= g_tol).all())
  finally:
    st.losses.FUSED_LOSS, hip_lib.flow_loss_f32 = saved_fused, saved_entry
  # the network inputs of the two paths: x_t to the rounding of a y + t n (k = 2, and one for a = 1 - t), the time labels alike
  t64 = t.astype(np.float64)
  x_want = w(1. - t64) * y + w(t64) * n64
  x_mag = w(1. - t64) * np.abs(y) + w(t64) * np.abs(n64)
  for fused in (True, False):
    within(seen[fused][0], x_want, x_mag, 4, f'{family} fused={fused} x_t')
    assert torch.equal(seen[fused][1], t_dev if family == 've' else t_dev * 999), f'{family} fused={fused}: the time labels'
  assert torch.equal(seen[True][0], seen[False][0]), 'stk_perturb_f32 and the torch expression differ in x_t'


# ---- the loop with the closed-form Gaussian velocity ------------------------------------------------------------------------
LOOP_STEPS = 50
LOOP_CASES = {'order1': dict(order=1), 'order2': dict(order=2), 'eta0.7': dict(order=1, eta=0.7)}


@pytest.fixture(scope='module')
def gaussian_reference(st):
  """Per case: the schedule, the start state (fp32), the recorded noise, the float64 restatement's result and the same in
  numpy fp32.  Computed once."""
  shape = (4, 3, 8, 8)
  rng = np.random.RandomState(0)
  c = rng.uniform(0.3, 2., size=shape).astype(np.float32).astype(np.float64)
  x1 = np.random.RandomState(1).standard_normal(shape).astype(np.float32)
  v_of = R.gaussian_velocity(c)
  out = {}
  for name, opts in LOOP_CASES.items():
    sch = st.flow.flow_schedule(LOOP_STEPS, shift=3., **opts)
    rng = np.random.RandomState(5)
    noise = [rng.standard_normal(shape).astype(np.float32) for _ in range(int((sch.rows[:, 2] > 0).sum()))]
    x64 = R.loop(sch, v_of, x1, noise=noise)
    x32 = R.loop(sch, v_of, x1, noise=noise, dtype=np.float32)
    assert x32.dtype == np.float32
    out[name] = dict(c=c, x1=x1, sch=sch, noise=noise, x64=x64, x32=x32)
  return out


class _Counted:
  """Counts the launches of the step entry on a library for the length of a `with`."""

  def __init__(self, lib):
    self.lib, self.n = lib, dict(step=0)

  def __enter__(self):
    self.saved = self.lib.flow_step_f32
    self.lib.flow_step_f32 = lambda *a: (self.n.__setitem__('step', self.n['step'] + 1), self.saved(*a))[1]
    return self.n

  def __exit__(self, *exc):
    self.lib.flow_step_f32 = self.saved
    return False


def _device_velocity(c, dev):
  """The closed-form velocity of _flow_ref.gaussian_velocity by torch fp32 operators in the same order."""
  c2 = torch.from_numpy((c * c).astype(np.float32)).to(dev)

  def v_of(x, t):
    tt = t[0]
    a = 1. - tt
    return (tt - a * c2) / (a * a * c2 + tt * tt) * x
  return v_of


@pytest.mark.parametrize('case', list(LOOP_CASES))
def test_loop_with_the_closed_form_gaussian_velocity(st, hip_lib, gaussian_reference, case):
  ref = gaussian_reference[case]
  sch = ref['sch']
  dev = torch.device('cuda:0')
  field = _device_velocity(ref['c'], dev)
  heun = sch.order == 2
  levels = ([float(t) for pair in zip(sch.times[:-1], sch.times[1:]) for t in pair][:sch.nfe] if heun else [float(t) for t in sch.times[:-1]])
  calls = []

  def velocity_fn(x, t):
    assert t.shape == (4,) and t.dtype == torch.float32 and t.device == x.device
    assert bool((t == f32(levels[len(calls)])).all()), (float(t[0]), levels[len(calls)])     # exactly the schedule's times, in order
    calls.append(float(t[0]))
    return field(x, t)

  noise = iter(torch.from_numpy(e).to(dev) for e in ref['noise'])
  x = torch.from_numpy(ref['x1']).to(dev)
  with _Counted(hip_lib) as count:
    out = st.flow.flow_sample(velocity_fn, sch, x, noise_fn=lambda v: next(noise))
  assert out is x, 'the state was not advanced in place'
  assert len(calls) == sch.nfe == (2 * LOOP_STEPS - 1 if heun else LOOP_STEPS) and count['step'] == sch.launches == sch.nfe
  assert 0. not in calls, 'the velocity was evaluated at t = 0'
  assert len(ref['noise']) == (LOOP_STEPS - 1 if case == 'eta0.7' else 0) and next(noise, None) is None, 'not every recorded eps was drawn'
  got = out.cpu().double().numpy()
  own = R.rel(ref['x32'], ref['x64'])
  err = R.rel(got, ref['x64'])
  print(f'{case}: product loop deviates {err:.2e} from the float64 restatement; the restatement in numpy fp32 deviates {own:.2e}: '
        f'tolerance {4 * own:.2e}')
  assert err <= 4 * own
  if case == 'order2':
    # the exact map of Gaussian data is x(0) = c x(1); the float64 loop misses it by the variance recursion's error exactly
    exact = ref['c'] * ref['x1'].astype(np.float64)
    var = R.variance_recursion(sch, ref['c'])
    assert np.allclose(ref['x64'], np.sqrt(var) * ref['x1'], rtol=1e-10, atol=0)
    rec = float(np.abs((np.sqrt(var) - ref['c']) * ref['x1']).max() / np.abs(exact).max())
    print(f'{case}: error against the exact map {R.rel(got, exact):.3e}; the variance recursion allows {rec:.3e}')
    assert R.rel(got, exact) <= rec + 4 * own


# ---- the sampler on the tiny networks ---------------------------------------------------------------------------------------
STEPS = 6


def _shape(cfg):
  return (2, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)


def _sampler(st, cfg, sde, **options):
  c = copy.deepcopy(cfg)
  c.sampling.flow_steps = STEPS
  for k, v in options.items():
    setattr(c.sampling, k, v)
  return st.sampling.get_sampling_fn(c, sde, _shape(c), st.datasets.get_data_inverse_scaler(c), 1e-3)


def _by_hand(st, cfg, sde, model, dtype, seed, velocity=None, **opts):
  """The test's own loop: the same engine network, the updates in torch `dtype` from the schedule's rows."""
  sch = st.flow.flow_schedule(STEPS, **opts)
  v_fn = velocity or st.models.utils.get_flow_model_fn(cfg, model, train=False)
  c = (lambda v: float(v)) if dtype == torch.float64 else f32
  torch.manual_seed(seed)
  with torch.no_grad():
    x = sde.prior_sampling(_shape(cfg)).to(cfg.device).to(dtype)
    ones = torch.ones(x.shape[0], device=x.device)
    net = lambda xx, t: v_fn(xx.float().contiguous(), ones * f32(t)).to(dtype)
    for i in range(sch.steps):
      cx, cv, cn = (c(v) for v in sch.rows[i])
      v = net(x, sch.times[i])
      if sch.order == 2 and i < sch.steps - 1:
        x1 = cx * x + cv * v
        x = cx * x + cv * (0.5 * v + 0.5 * net(x1, sch.times[i + 1]))
        continue
      xn = cx * x + cv * v
      if sch.rows[i][2] > 0.:
        xn = xn + cn * torch.randn_like(x.float()).to(dtype)
      x = xn
    return st.datasets.get_data_inverse_scaler(cfg)(x)


def _rel(a, b):
  return R.rel(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy())


SAMPLER_CASES = {'order1': dict(order=1), 'order2': dict(order=2), 'shifted-eta': dict(order=1, shift=3., eta=0.7)}


@pytest.mark.parametrize('case', list(SAMPLER_CASES))
@pytest.mark.parametrize('family', ['vp', 've'], ids=['positional', 'fourier'])
def test_sampler_matches_a_float64_loop(st, hip_lib, family, case):
  cfg, sde, model = _tiny(st, hip_lib, family)
  opts = SAMPLER_CASES[case]
  fn = _sampler(st, cfg, sde, **{'flow_' + k: v for k, v in opts.items()})
  sch = st.flow.flow_schedule(STEPS, **opts)
  evals = []
  hook = model.module.register_forward_hook(lambda m, a, o: evals.append(1))
  try:
    torch.manual_seed(3)
    with _Counted(hip_lib) as count:
      got, nfe = fn(model)
  finally:
    hook.remove()
  assert nfe == sch.nfe == len(evals) == (2 * STEPS - 1 if opts['order'] == 2 else STEPS) and count['step'] == sch.launches == nfe
  assert got.shape == _shape(cfg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again), 'two runs under one seed differ'
  want = _by_hand(st, cfg, sde, model, torch.float64, 3, **opts)
  own = _rel(_by_hand(st, cfg, sde, model, torch.float32, 3, **opts), want)
  err = _rel(got, want)
  print(f'{family} {case}: sampler deviates {err:.2e} from the float64 loop; the same loop in torch fp32 deviates {own:.2e}: '
        f'tolerance {4 * own:.2e}')
  assert err <= 4 * own


def _rng_states():
  return torch.get_rng_state(), torch.cuda.get_rng_state()


@pytest.mark.parametrize('eta', [0., 0.7])
def test_the_draws_of_a_run(st, hip_lib, eta):
  """At eta = 0 the generators after a whole run are where one sde.prior_sampling(shape) alone leaves them; at eta > 0 where
  steps - 1 further torch.randn_like of the state leave them (their order is what test_sampler_matches_a_float64_loop holds)."""
  cfg, sde, model = _tiny(st, hip_lib, 'vp')
  fn = _sampler(st, cfg, sde, flow_eta=eta)
  torch.manual_seed(5)
  fn(model)
  after_run = _rng_states()
  torch.manual_seed(5)
  x = sde.prior_sampling(_shape(cfg)).to(cfg.device)
  after_prior = _rng_states()
  for _ in range(STEPS - 1 if eta > 0 else 0):
    torch.randn_like(x)
  after_draws = _rng_states()
  torch.manual_seed(5)
  untouched = _rng_states()
  assert torch.equal(after_run[0], after_draws[0]) and torch.equal(after_run[1], after_draws[1])
  assert not (torch.equal(after_prior[0], untouched[0]) and torch.equal(after_prior[1], untouched[1])), 'the prior drew nothing'
  assert (eta > 0) == (not torch.equal(after_draws[1], after_prior[1])), 'the noise of the steps comes from the device generator'


@pytest.mark.parametrize('c', [0.5, 2.])
def test_rk45_on_the_closed_form_field(st, hip_lib, c):
  """order = 'rk45' on x_0 ~ N(0, c^2), c in {0.5, 2} (the two data laws of the derivation): the solver on the device, the field
  on the float32 cast of its state, takes the evaluations the same solver takes in float64 on the CPU, and agrees with it under
  the measured rule (the CPU solver on the fp32 field is the yardstick).  Equal counts are a statement about these fields: the
  step controller is continuous in the error estimate but for its accept / reject decision, so the counts agree where no
  decision lies within the fp32 noise of the estimate, a few per cent at rtol = atol = 1e-5 (RK45 takes steps of 0.1 - 0.4
  here)."""
  dev = torch.device('cuda:0')
  shape = (4, 3, 8, 8)
  cs = np.full(shape, c)
  x1 = torch.randn(shape, generator=torch.Generator().manual_seed(1))
  c2_64 = torch.from_numpy(cs * cs)

  def field64(t, y):
    a = 1. - t
    return ((t - a * c2_64) / (a * a * c2_64 + t * t)).reshape(-1) * y

  host32 = _device_velocity(cs, torch.device('cpu'))
  solve = st.engine.rk45.solve_ivp_rk45
  want, nfev64 = solve(field64, (1., 1e-3), x1.reshape(-1).double(), rtol=1e-5, atol=1e-5)
  cast = lambda t, y: host32(y.reshape(shape).float(), torch.full((4,), float(t))).reshape(-1).double()
  own_y, nfev32 = solve(cast, (1., 1e-3), x1.reshape(-1).double(), rtol=1e-5, atol=1e-5)
  with _Counted(hip_lib) as count:
    got, nfev = st.flow.flow_solve_rk45(_device_velocity(cs, dev), x1.to(dev))
  assert count['step'] == 0, "order = 'rk45' launched a kernel of the header"
  assert got.dtype == torch.float32 and got.shape == shape
  own = R.rel(own_y.numpy(), want.numpy())
  err = R.rel(got.cpu().double().numpy().reshape(-1), want.numpy())
  exact = R.rel(want.numpy(), (np.sqrt(0.999 ** 2 * c * c + 1e-6) * x1.double().numpy()).reshape(-1))
  print(f'rk45 c={c}: nfev {nfev} on the device, {nfev64} in float64 on the CPU ({nfev32} with the fp32 field there); deviates '
        f'{err:.2e}, the CPU solver on the fp32 field {own:.2e}: tolerance {4 * own:.2e}; float64 against the exact flow {exact:.2e}')
  assert nfev == nfev64
  assert err <= 4 * own


def test_rk45_sampler_on_a_tiny_network(st, hip_lib):
  cfg, sde, model = _tiny(st, hip_lib, 'vp')
  fn = _sampler(st, cfg, sde, flow_order='rk45', flow_t_end=0.5, flow_rtol=1e-3, flow_atol=1e-3)
  evals = []
  hook = model.module.register_forward_hook(lambda m, a, o: evals.append(1))
  try:
    torch.manual_seed(3)
    with _Counted(hip_lib) as count:
      got, nfe = fn(model)
  finally:
    hook.remove()
  assert nfe == len(evals) >= 8 and count['step'] == 0
  assert got.shape == _shape(cfg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  with pytest.raises(ValueError, match='fp16'):
    _sampler(st, cfg, sde, flow_order='rk45', precision='fp16')


def test_guided_run_is_the_loop_on_the_guided_velocity(st, hip_lib):
  """A run under class_condition(model, y, 1.5) is the loop fed v_c + 1.5 (v_c - v_u): guidance acts inside the model."""
  cfg, sde, model = _tiny(st, hip_lib, 'vp', num_classes=3)
  mutils = st.models.utils
  y, w = [2, 0], 1.5
  fn = _sampler(st, cfg, sde, flow_order=2)
  torch.manual_seed(3)
  with mutils.class_condition(model, y, w):
    got, nfe = fn(model)
  assert nfe == 2 * STEPS - 1
  torch.manual_seed(3)
  with mutils.class_condition(model, y, 0.):
    plain, _ = fn(model)
  assert not torch.equal(got, plain), 'the guidance changed nothing'
  v_fn = mutils.get_flow_model_fn(cfg, model, train=False)

  def guided(dtype):
    """The two evaluations in fp32, the combination in `dtype`."""
    def velocity(x, t):
      with mutils.class_condition(model, y, 0.):
        c = v_fn(x, t).to(dtype)
      with mutils.class_condition(model, [None, None], 0.):
        u = v_fn(x, t).to(dtype)
      return c + w * (c - u)
    return velocity

  want = _by_hand(st, cfg, sde, model, torch.float64, 3, velocity=guided(torch.float64), order=2)
  own = _rel(_by_hand(st, cfg, sde, model, torch.float32, 3, velocity=guided(torch.float32), order=2), want)
  err = _rel(got, want)
  print(f'guided: sampler deviates {err:.2e} from the float64 loop on the guided velocity; the same loop in torch fp32 deviates '
        f'{own:.2e}: tolerance {4 * own:.2e}')
  assert err <= 4 * own


def test_fp16_runs(st, hip_lib):
  """precision = 'fp16' (the network only): finite samples, the same counts, and a difference from the fp32 run that stays
  within what the EDM sampler shows between its own fp32 and fp16 runs.  That yardstick is measured here, not fixed: the run of
  tests/test_gpu_edm.py::test_fp16_runs -- the same wide network (same seed, same weights) under configs.edm, 6 Heun steps,
  the same 11 evaluations as the 6 Heun steps of the flow sampler, the same seed of the prior.  Both figures are printed."""
  cfg, sde, model = _tiny(st, hip_lib, 'wide')
  outs = {}
  for precision in ('fp32', 'fp16'):
    torch.manual_seed(9)
    with _Counted(hip_lib) as count:
      outs[precision], nfe = _sampler(st, cfg, sde, flow_order=2, precision=precision)(model)
    assert nfe == 2 * STEPS - 1 and count['step'] == nfe and bool(torch.isfinite(outs[precision]).all())
  diff = float((outs['fp16'] - outs['fp32']).abs().max())
  # the yardstick: the EDM sampler's own pair
  e_cfg, _, e_sde, e_model, _ = build_pair(st, st.configs.edm(tiny_config(st, 'wide')), hip_lib)
  e_model.eval()
  e_outs = {}
  for precision in ('fp32', 'fp16'):
    c = copy.deepcopy(e_cfg)
    c.sampling.edm_steps, c.sampling.precision = STEPS, precision
    torch.manual_seed(9)
    e_outs[precision], e_nfe = st.sampling.get_sampling_fn(c, e_sde, _shape(c), st.datasets.get_data_inverse_scaler(c), 1e-3)(e_model)
    assert e_nfe == nfe and bool(torch.isfinite(e_outs[precision]).all())
  e_diff = float((e_outs['fp16'] - e_outs['fp32']).abs().max())
  print(f'wide: fp16 against fp32 after {nfe} evaluations: max |difference| {diff:.3e}; the EDM sampler on the same network: {e_diff:.3e}')
  assert diff > 0, 'the fp16 mode did not reach the network'
  assert e_diff > 0 and diff <= e_diff, f'fp16 deviates {diff:.3e} from fp32, the EDM sampler {e_diff:.3e}'
