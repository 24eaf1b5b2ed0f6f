"""Host side of rectified flow: sde_lib.RectifiedFlow and its refusals, the velocity and score functions' conditioning, the
schedule of flow.py against the restatement of tests/_flow_ref.py, the derivation of the step's row on Gaussian data, the
torch-expression loss on the tiny network (checker library) against a float64 restatement, the training step, the ctypes
table of include/stk_flow.h, the refusal of host tensors and of a library without the header, and the dispatch of
get_sampling_fn and get_loss_fn.  No GPU.

The derivation.  For x_0 ~ N(0, c^2) the exact velocity is k(t) x (_flow_ref.gaussian_k), so the sampler's variance obeys a
scalar recursion (_flow_ref.variance_recursion) whose fixed point must be the data's c^2.  Figures of this file's own run
(float64; c in {0.5, 2}, shift in {1, 3}, eta in {0, 0.5, 1}): relative error of the final variance at 1000 steps at most
5.8e-3 for order 1 (shift 3, c 0.5, eta 0) and 3.7e-5 for order 2; error(1000) / error(50) between 0.051 and 0.055 for order
1: first order.  A wrong sign or factor in cx, cv or cn misses c^2 by orders of magnitude.

The loss tolerance.  As tests/test_edm_cpu.py: the loss is compared with a float64 restatement on the network output F the same
tiny network (checker library, fp32) gives at the restatement's own network input, rounded to fp32, so what differs is fp32
rounding alone; held to F32_FWD_RTOL of tests/_tolerances.py, relative to the largest loss of the batch, and the gradient
with respect to F relative to its largest entry.
"""
import copy
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _flow_ref as R
from _model_util import build_pair, make_state, patched_rng, tiny_config
from _tolerances import F32_FWD_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['stk_flow_ws_bytes', 'stk_flow_loss_f32', 'stk_flow_loss_grad_f32', 'stk_flow_step_f32']


@pytest.fixture
def flow(st):
  return st.flow


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def _cfg(st, family='vp', **options):
  return st.configs.flow(tiny_config(st, family), **options)


def test_module_is_part_of_the_package(st, flow):
  assert 'flow' in st.__all__ and st._REFERENCE_NAMES['flow'] is flow
  for name in ('flow_schedule', 'flow_sample', 'get_flow_sampler', 'sampling_options', 'FlowSchedule'):
    assert callable(getattr(flow, name)), name
  assert st.models.utils.get_velocity_fn is st.models.utils.get_flow_model_fn


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_flow.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_flow.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_FLOW
  assert sorted(n for n, _ in decls) == sorted(table) == sorted(ENTRIES)
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.has == 'has_flow']
  assert len(row) == 1 and row[0].path == 'include/stk_flow.h' and row[0].table is table
  assert row[0].restype == {'stk_flow_ws_bytes': L.c_long} and tuple(row[0].unchecked) == ()
  order = [h.has for h in L.OPTIONAL_HEADERS]
  assert order[order.index('has_parallel') + 1] == 'has_flow' and order[order.index('has_augment') + 1] == 'has_parallel'
  assert order[-3:] == ['has_consistency', 'has_edm', 'has_guided']
  for name in table:
    assert name not in open(os.path.join(ROOT, 'include', 'stk.h')).read()
    assert name not in open(os.path.join(ROOT, 'oracle', 'stk_ref.c')).read()


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_flow is True and ref_lib.has_flow is False
  assert not hasattr(ref_lib, 'flow_step_f32')
  assert getattr(lib.flow_step_f32, 'raw', None) is not None and not hasattr(lib.flow_ws_bytes, 'raw')


def test_workspace_query_answers_without_a_device(st):
  lib = st.engine.lib.load()
  EINVAL, EUNSUPPORTED = -1, -3
  assert lib.flow_ws_bytes(0, 16) == EINVAL and lib.flow_ws_bytes(-3, 16) == EINVAL and lib.flow_ws_bytes(2, 0) == EINVAL
  assert lib.flow_ws_bytes(2, 2 ** 30) == EUNSUPPORTED and lib.flow_ws_bytes(1, 2 ** 31) == EUNSUPPORTED
  assert lib.flow_ws_bytes(1, 2 ** 31 - 4) > 0
  # as stk_edm_ws_bytes: one float64 per (sample, block)
  for B, inner in ((128, 3072), (3000, 4), (1, 1), (4, 3 * 256 * 256), (16, 3 * 256 * 256)):
    assert lib.flow_ws_bytes(B, inner) == lib.edm_ws_bytes(B, inner) > 0


# ---- the family -------------------------------------------------------------------------------------------------------
def test_get_sde_and_the_family(st):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.training.sde = 'rectified_flow'
  sde = st.sde_lib.get_sde(cfg, None)
  assert isinstance(sde, st.sde_lib.RectifiedFlow) and isinstance(sde, st.sde_lib._GaussianPrior)
  assert sde.T == 1 and sde.eps == 1e-3 and sde.get_t_min(cfg) == 1e-3 and sde._prior_scale == 1
  x = torch.randn(3, 2, 4, 4, generator=torch.Generator().manual_seed(0))
  t = torch.tensor([0.001, 0.5, 1.0], dtype=torch.float64)
  mean, std = sde.marginal_prob(x.double(), t)
  assert mean.dtype == std.dtype == torch.float64 and torch.equal(std, t)
  assert torch.equal(mean, (1. - t)[:, None, None, None] * x.double()) and not mean[2].any()
  mean32, std32 = sde.marginal_prob(x, t.float())
  assert mean32.dtype == std32.dtype == torch.float32
  # the equivalent diffusion: drift -x / (1 - t), diffusion sqrt(2 t / (1 - t)); singular at t = 1, and documented as such
  drift, g = sde.sde(x[:2].double(), t[:2])
  assert torch.allclose(drift, -x[:2].double() / (1. - t[:2])[:, None, None, None], rtol=1e-14)
  assert torch.allclose(g, torch.sqrt(2. * t[:2] / (1. - t[:2])), rtol=1e-14)
  assert not bool(torch.isfinite(sde.sde(x[2:].double(), t[2:])[1]).all())
  assert 'singular' in st.sde_lib.RectifiedFlow.__doc__.lower()
  # g^2 / 2 = d/dt (std^2) / 2 - (d/dt ln alpha) std^2 with alpha = 1 - t, std = t: the marginals are the interpolant's
  tt = t[:2]
  assert torch.allclose(g ** 2, 2. * tt + 2. * tt * tt / (1. - tt), rtol=1e-12)
  torch.manual_seed(1)
  z = sde.prior_sampling((2, 3, 4, 4))
  torch.manual_seed(1)
  assert torch.equal(z, torch.randn(2, 3, 4, 4))
  want = -48 / 2. * np.log(2 * np.pi) - (z.double() ** 2).sum(dim=(1, 2, 3)) / 2.
  assert torch.allclose(sde.prior_logp(z).double(), want, rtol=1e-6)


REFUSALS = [('model', 'scale_by_sigma', True), ('training', 'continuous', False)]
TRAINING_REFUSALS = [('training', k, True) for k in ('mixed', 'importance_sampling', 'likelihood_weighting', 'reconstruction_loss')]


@pytest.mark.parametrize('section,key,value', REFUSALS + TRAINING_REFUSALS, ids=lambda v: str(v))
def test_refusals_name_the_key(st, product_backend, section, key, value):
  """Each refusal is a ValueError naming the key, raised when the step function, the loss or the sampler is built."""
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  check = st.models.utils.check_flow_config
  check(cfg), check(cfg, training=True)
  assert callable(st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg)))
  assert callable(st.flow.get_flow_sampler(cfg, sde, (2, 3, 16, 16), lambda v: v))
  setattr(getattr(cfg, section), key, value)
  with pytest.raises(ValueError, match=key):
    check(cfg, training=True)
  with pytest.raises(ValueError, match=key):
    st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  with pytest.raises(ValueError, match=key):
    st.losses.get_flow_loss_fn(cfg, sde, True)
  if (section, key, value) in REFUSALS:
    with pytest.raises(ValueError, match=key):
      check(cfg)
    with pytest.raises(ValueError, match=key):
      st.flow.get_flow_sampler(cfg, sde, (2, 3, 16, 16), lambda v: v)
    with pytest.raises(ValueError, match=key):
      st.sampling.get_sampling_fn(cfg, sde, (2, 3, 16, 16), lambda v: v, 1e-3)
    with pytest.raises(ValueError, match=key):
      st.models.utils.get_score_fn(cfg, sde, None, train=False, continuous=True)
    with pytest.raises(ValueError, match=key):
      st.models.utils.get_raw_fn(cfg, sde, None, train=False, continuous=True)
    with pytest.raises(ValueError, match=key):
      st.models.utils.get_velocity_fn(cfg, None, train=False)
  else:
    check(cfg)                                          # a sampler does not mind the training switches


def test_centred_and_uncentred_data_are_both_allowed(st):
  for centered in (True, False):
    cfg = _cfg(st)
    cfg.data.centered = centered
    st.models.utils.check_flow_config(cfg, training=True)


def test_configs_flow(st):
  for name, make in st.configs.BASELINE_CONFIGS.items():
    base = make()
    cfg = st.configs.flow(base)
    assert base.training.sde != 'rectified_flow' and 'flow_time' not in base.training, 'the shipped config was changed in place'
    assert cfg.training.sde == 'rectified_flow' and cfg.sampling.method == 'flow' and cfg.training.continuous is True
    assert cfg.model.scale_by_sigma is False and cfg.data.centered == base.data.centered
    assert (cfg.training.flow_time, cfg.training.flow_p_mean, cfg.training.flow_p_std) == ('logit_normal', 0., 1.)
    assert st.flow.sampling_options(cfg) == (50, 1, 1., 0., 1e-3, 1e-5, 1e-5)
    st.models.utils.check_flow_config(cfg, training=True)
    assert isinstance(st.sde_lib.get_sde(cfg, None), st.sde_lib.RectifiedFlow), name
  cfg = st.configs.flow(st.configs.cifar10_ddpmpp_nll_st(), steps=25, order=2, shift=3., eta=0., p_mean=-0.5, p_std=1.5)
  assert st.flow.sampling_options(cfg)[:4] == (25, 2, 3., 0.) and (cfg.training.flow_p_mean, cfg.training.flow_p_std) == (-0.5, 1.5)


# ---- the schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('eta', [0., 0.7])
@pytest.mark.parametrize('shift', [1., 3.])
@pytest.mark.parametrize('steps', [1, 2, 7, 50])
def test_schedule_is_the_restatement(flow, steps, shift, eta, order):
  if eta > 0. and order == 2:
    with pytest.raises(ValueError, match='eta'):
      flow.flow_schedule(steps, order=order, shift=shift, eta=eta)
    return
  s = flow.flow_schedule(steps, order=order, shift=shift, eta=eta)
  t = R.times(steps, shift)
  assert s.times.dtype == s.delta.dtype == s.rows.dtype == np.float64
  assert np.array_equal(s.times, t) and np.array_equal(s.times, s.times.astype(np.float32).astype(np.float64))
  assert s.times[0] == 1. and s.times[-1] == 0. and bool((np.diff(s.times) < 0).all())
  assert np.array_equal(s.delta, t[:-1] - t[1:])
  want = R.rows(t, eta)
  assert s.rows.shape == (steps, 3) and np.allclose(s.rows, want, rtol=1e-15, atol=0)
  assert tuple(s.rows[-1]) == (1., -t[-2], 0.), 'the last step is not the plain Euler step to t = 0'
  if eta == 0.:
    assert bool((s.rows[:, 0] == 1.).all()) and bool((s.rows[:, 2] == 0.).all()) and np.array_equal(s.rows[:, 1], -s.delta)
  else:
    assert bool((s.rows[:-1, 2] > 0.).all()) and bool((s.rows[:, 0] > 0.).all())
  assert s.nfe == (steps if order == 1 else 2 * steps - 1) and s.launches == s.nfe
  assert (s.steps, s.order, s.shift, s.eta) == (steps, order, shift, eta)
  if shift == 1.:
    assert np.array_equal(s.times, R.fp32(1. - np.arange(steps + 1) / steps)), 'shift = 1 is not the uniform grid'
  else:
    assert bool((s.times[1:-1] > (1. - np.arange(steps + 1) / steps)[1:-1]).all()), 'shift > 1 does not move the times up'


def test_bad_options_name_the_option(flow):
  for steps in (0, 2.5, -3, True, 'many', None, float('inf'), float('-inf'), float('nan')):
    with pytest.raises(ValueError, match='steps'):
      flow.flow_schedule(steps)
  for order in (0, 3, 'heun', None, True, 1.5, np.int64(3)):
    with pytest.raises(ValueError, match='order'):
      flow.flow_schedule(10, order=order)
  numpy_ints = flow.flow_schedule(np.int64(10), order=np.int64(2))         # a config may hold numpy integers
  assert (numpy_ints.steps, numpy_ints.order, numpy_ints.nfe) == (10, 2, 19) and type(numpy_ints.order) is int
  for shift in (0., -1., float('inf'), float('nan')):
    with pytest.raises(ValueError, match='shift'):
      flow.flow_schedule(10, shift=shift)
  for eta in (-0.1, float('inf'), float('nan')):
    with pytest.raises(ValueError, match='eta'):
      flow.flow_schedule(10, eta=eta)
  for order in (2, 'rk45'):
    with pytest.raises(ValueError, match='eta'):
      flow.flow_schedule(10, order=order, eta=0.5)
  with pytest.raises(ValueError, match='eta'):                # eta max D >= 1: cx would not be positive
    flow.flow_schedule(2, eta=2.)
  with pytest.raises(ValueError, match='eta'):
    flow.flow_schedule(1, eta=1.)
  flow.flow_schedule(2, eta=1.9)
  with pytest.raises(ValueError, match='coincide'):          # shift 1e10 puts t_1 within 1e-10 of 1: it rounds to t_0 in fp32
    flow.flow_schedule(2, shift=1e10)


# ---- the derivation, on a Gaussian data law ---------------------------------------------------------------------------
def _variance_error(flow, steps, order, shift, eta, c):
  s = flow.flow_schedule(steps, order=order, shift=shift, eta=eta)
  return abs(R.variance_recursion(s, c) - c * c) / (c * c)


@pytest.mark.parametrize('shift', [1., 3.])
@pytest.mark.parametrize('c', [0.5, 2.])
def test_rows_keep_the_marginals_of_gaussian_data(flow, c, shift):
  """The package's rows, in the float64 variance recursion of the restatement, reach the data's variance: below 1e-2 at 1000
  steps and below a tenth of the error at 50 (first order) for every eta; below 1e-4 for Heun."""
  for eta in (0., 0.5, 1.):
    e50, e1000 = (_variance_error(flow, n, 1, shift, eta, c) for n in (50, 1000))
    print(f'c={c} shift={shift} eta={eta}: order 1 error {e50:.3e} at 50 steps, {e1000:.3e} at 1000, ratio {e1000 / e50:.4f}')
    assert e1000 < 1e-2 and e1000 < 0.1 * e50
  h50, h1000 = (_variance_error(flow, n, 2, shift, 0., c) for n in (50, 1000))
  print(f'c={c} shift={shift}: order 2 error {h50:.3e} at 50 steps, {h1000:.3e} at 1000')
  assert h1000 < 1e-4


def test_the_recursion_is_the_loop(flow):
  """The scalar recursion states what the loop does: the restated loop on per-element Gaussian data, fed unit-variance
  states, multiplies each element by the recursion's multiplier (eta = 0)."""
  c = 0.7
  x = np.random.RandomState(0).standard_normal((2, 3, 4, 4))
  for order in (1, 2):
    s = flow.flow_schedule(20, order=order, shift=3.)
    got = R.loop(s, R.gaussian_velocity(np.full(x.shape, c)), x)
    assert np.allclose(got * got, R.variance_recursion(s, c) * x * x, rtol=1e-10)
  # ... and the package's schedule drives the restated loop exactly as the restatement's own
  for order, eta in ((1, 0.), (2, 0.), (1, 0.7)):
    noise = [np.random.RandomState(i).standard_normal(x.shape) for i in range(19)] if eta else None
    a = R.loop(flow.flow_schedule(20, order=order, shift=3., eta=eta), R.gaussian_velocity(c), x, noise=noise)
    b = R.loop(R.Schedule(20, order, 3., eta), R.gaussian_velocity(c), x, noise=noise)
    assert R.rel(a, b) <= 1e-14


# ---- the velocity, the score and the loss on the tiny network (checker library) ---------------------------------------------
class _Tap(torch.nn.Module):
  """Records what the loss hands to the network and keeps the gradient of what it returns."""

  def __init__(self, inner):
    super().__init__()
    self.inner = inner
    self.seen = []

  def forward(self, x, cond):
    out = self.inner(x, cond)
    if out.requires_grad:
      out.retain_grad()
    self.seen.append((x.detach().clone(), cond.detach().clone(), out))
    return out


class _Stub(torch.nn.Module):
  """A network in closed form: out = 0.3 x + 0.001 labels."""

  def forward(self, x, labels):
    return 0.3 * x + 0.001 * labels[:, None, None, None]


@pytest.fixture(scope='module')
def tiny(st, ref_lib):
  out = {}
  for family in ('vp', 've'):                       # positional and fourier conditioning
    cfg, _, sde, model, _ = build_pair(st, _cfg(st, family), ref_lib)
    out[family] = (cfg, sde, model)
  return out


@pytest.mark.parametrize('family', ['vp', 've'])
def test_score_fn_is_the_velocity_formula_on_a_stub(st, family):
  """v = the raw network under 999 t (positional) or t (fourier); score = -(x + (1 - t) v) / t; raw_fn = (v, False)."""
  cfg = _cfg(st, family)
  sde = st.sde_lib.get_sde(cfg, None)
  model = _Stub()
  scale = 1. if cfg.model.embedding_type == 'fourier' else 999.
  x = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(2)).double()
  t = torch.tensor([1e-3, 0.4, 1.0], dtype=torch.float64)
  w = lambda v: v[:, None, None, None]
  v = st.models.utils.get_velocity_fn(cfg, model, train=False)(x, t)
  assert torch.allclose(v, 0.3 * x + 0.001 * w(t * scale), rtol=1e-14)
  raw, neg = st.models.utils.get_raw_fn(cfg, sde, model, train=False, continuous=True)
  assert neg is False and torch.equal(raw(x, t), v)
  x.requires_grad_(True)
  score = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=True)(x, t)
  want = -(x + w(1. - t) * v) / w(t)
  assert torch.allclose(score, want, rtol=1e-13)
  assert torch.equal(score[2], -x[2] / 1.), 'at t = 1 the score is that of the prior'
  grad, = torch.autograd.grad(score.sum(), x)                 # torch operators: autograd sees it
  assert torch.allclose(grad, w(-(1. + (1. - t) * 0.3) / t).expand_as(x), rtol=1e-13)


@pytest.mark.parametrize('family', ['vp', 've'])
def test_velocity_fn_conditions_the_tiny_network(st, tiny, family):
  cfg, sde, model = tiny[family]
  tap = _Tap(model)
  x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(2))
  t = torch.tensor([0.05, 0.5, 1.0])
  with torch.no_grad():
    v = st.models.utils.get_flow_model_fn(cfg, tap, train=False)(x, t)
  x_in, cond, F = tap.seen[0]
  assert torch.equal(x_in, x) and torch.equal(F, v)
  assert torch.equal(cond, t if cfg.model.embedding_type == 'fourier' else t * 999)


@pytest.mark.parametrize('time_law', ['logit_normal', 'uniform'])
@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_torch_loss_matches_the_float64_restatement(st, tiny, family, reduce_mean, time_law):
  cfg, sde, model = tiny[family]
  cfg = copy.deepcopy(cfg)
  cfg.training.reduce_mean = reduce_mean
  cfg.training.flow_time = time_law
  cfg.training.flow_p_mean, cfg.training.flow_p_std = -0.3, 1.2
  tap = _Tap(model)
  B = 5
  batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(3))
  loss_fn = st.losses.get_flow_loss_fn(cfg, sde, True)
  model.zero_grad()
  with patched_rng(17):
    losses = loss_fn(tap, batch, importance_sampling=None, t_min=None)
  assert losses.shape == (B,) and losses.dtype == torch.float32
  go = torch.randn(B, generator=torch.Generator().manual_seed(4))
  (losses * go).sum().backward()
  x_in, cond, F = tap.seen[0]
  # the draw order: one [B] draw for the time first, randn_like(batch) second
  with patched_rng(17):
    if time_law == 'uniform':
      t32 = (1. - torch.rand(B)).numpy()
    else:
      t32 = torch.sigmoid(-0.3 + 1.2 * torch.randn(B)).numpy()
    n = torch.randn_like(batch).double().numpy()
  assert t32.dtype == np.float32 and bool((t32 > 0).all()) and bool((t32 <= 1).all())
  t = t32.astype(np.float64)
  y = batch.double().numpy()
  w = lambda v: v[:, None, None, None]
  want_in = w(1. - t) * y + w(t) * n
  assert R.rel(x_in.double().numpy(), want_in) <= 1e-6
  want_cond = t if cfg.model.embedding_type == 'fourier' else 999. * t
  assert np.allclose(cond.double().numpy(), want_cond, rtol=2e-7, atol=0)
  # the restatement on the network's answer to ITS OWN input
  with torch.no_grad():
    F64 = _Tap(model)(torch.from_numpy(want_in).float(), torch.from_numpy(want_cond).float()).double()
  Fv = F64.clone().requires_grad_(True)
  yv, nv = torch.from_numpy(y), torch.from_numpy(n)
  r = Fv - (nv - yv)
  total = (r * r).reshape(B, -1)
  want = total.mean(dim=1) if reduce_mean else total.sum(dim=1)
  assert np.allclose(want.detach().numpy(), R.loss(F64.numpy(), y, n, reduce_mean), rtol=1e-12)
  (want * go.double()).sum().backward()
  e_loss = float((losses.detach().double() - want.detach()).abs().max() / want.detach().abs().max())
  e_grad = float((F.grad.double() - Fv.grad).abs().max() / Fv.grad.abs().max())
  print(f'{family} reduce_mean={reduce_mean} {time_law}: loss {e_loss:.2e}, dLoss/dF {e_grad:.2e} (bound {F32_FWD_RTOL:.1e})')
  assert e_loss <= F32_FWD_RTOL and e_grad <= F32_FWD_RTOL
  assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in model.parameters()), 'no gradient reached the network'


@pytest.mark.parametrize('time_law', ['logit_normal', 'uniform'])
def test_draw_order_reproduces_under_a_seed(st, tiny, time_law):
  """One [B] draw, then one randn_like: nothing else moves torch's generator."""
  cfg, sde, model = tiny['vp']
  cfg = copy.deepcopy(cfg)
  cfg.training.flow_time = time_law
  batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(3))
  loss_fn = st.losses.get_flow_loss_fn(cfg, sde, False)
  seen = []
  for seed in (5, 5, 6):
    tap = _Tap(model)
    torch.manual_seed(seed)
    with torch.no_grad():
      losses = loss_fn(tap, batch)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    t = 1. - torch.rand(4) if time_law == 'uniform' else torch.sigmoid(0. + 1. * torch.randn(4))
    n = torch.randn_like(batch)
    assert torch.equal(torch.get_rng_state(), state), 'the loss drew something else as well'
    assert torch.equal(tap.seen[0][1], t * 999)
    want_in = (1. - t.double())[:, None, None, None] * batch.double() + t.double()[:, None, None, None] * n.double()
    assert R.rel(tap.seen[0][0].double().numpy(), want_in.numpy()) <= 1e-6
    seen.append(losses)
  assert torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


def test_uniform_time_never_yields_zero(st, tiny, monkeypatch):
  """t = 1 - rand with rand in [0, 1): the ends of torch.rand's range give t = 1 and t = 2^-24, never 0."""
  cfg, sde, model = tiny['vp']
  cfg = copy.deepcopy(cfg)
  cfg.training.flow_time = 'uniform'
  batch = st.datasets.synthetic_batch(cfg, 2, generator=torch.Generator().manual_seed(3))
  below_one = float(np.nextafter(np.float32(1), np.float32(0)))
  monkeypatch.setattr(torch, 'rand', lambda *size, device=None, **kw: torch.tensor([0., below_one], device=device))
  tap = _Tap(model)
  with torch.no_grad():
    losses = st.losses.get_flow_loss_fn(cfg, sde, False)(tap, batch)
  assert torch.equal(tap.seen[0][1], torch.tensor([1., 2. ** -24]) * 999) and bool(torch.isfinite(losses).all())


def test_loss_options_name_the_key(st):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  for bad in (0., -1., float('nan')):
    c = copy.deepcopy(cfg)
    c.training.flow_p_std = bad
    with pytest.raises(ValueError, match='flow_p_std'):
      st.losses.get_flow_loss_fn(c, sde, True)
  c = copy.deepcopy(cfg)
  c.training.flow_time = 'lognormal'
  with pytest.raises(ValueError, match='flow_time'):
    st.losses.get_flow_loss_fn(c, sde, True)
  for key in ('flow_time', 'flow_p_mean', 'flow_p_std'):       # absent keys: the defaults
    del cfg.training[key]
  assert callable(st.losses.get_flow_loss_fn(cfg, sde, True))


@pytest.mark.parametrize('micro', [1, 2])
def test_training_steps_move_parameters_and_ema(st, ref_lib, micro):
  base = _cfg(st)
  base.optim.num_micro_batch = micro
  base.optim.warmup = 2
  cfg, _, sde, model, _ = build_pair(st, base, ref_lib)
  state = make_state(st, cfg, model)
  state['optimizer']._backend = ref_lib
  state['ema'].set_backend(ref_lib)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  before = [p.detach().clone() for p in model.parameters()]
  ema_before = [s.detach().clone() for s in state['ema'].shadow_params]
  for i in range(2):
    batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(100 + i))
    with patched_rng(50 + i):
      losses = step_fn(state, batch)
    assert losses.shape == (4,) and bool(torch.isfinite(losses).all()) and bool((losses > 0).all())
  assert state['step'] == 2
  assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
  assert any(not torch.equal(a, b.detach()) for a, b in zip(ema_before, state['ema'].shadow_params))


# ---- refusals and dispatch ----------------------------------------------------------------------------------------------
def _no_model(x, c):
  raise AssertionError('the network was evaluated')


def test_loss_dispatch(st, monkeypatch):
  """get_loss_fn and get_step_fn choose the flow loss by the class of the sde."""
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  real = st.losses.get_flow_loss_fn
  monkeypatch.setattr(st.losses, 'get_flow_loss_fn', lambda *a: seen.append(a) or real(*a))
  assert callable(st.losses.get_loss_fn(cfg, sde, True))
  assert seen.pop() == (cfg, sde, True)
  st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  assert seen.pop() == (cfg, sde, True)
  assert st.losses._pick_loss_fn is st.losses.get_loss_fn, 'the earlier name is another function'
  # ... and no other family reaches it
  vp = tiny_config(st, 'vp')
  st.losses.get_loss_fn(vp, st.sde_lib.get_sde(vp, None), True)
  assert not seen
  with pytest.raises(ValueError, match='RectifiedFlow'):
    real(cfg, st.sde_lib.get_sde(vp, None), True)


def test_host_tensors_are_refused(st, flow, product_backend, monkeypatch):
  lib = product_backend.get()

  def no_launch(*a):
    raise AssertionError('a kernel was launched on host tensors')

  monkeypatch.setattr(lib, 'flow_step_f32', no_launch)
  for order in (1, 2):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      flow.flow_sample(_no_model, flow.flow_schedule(4, order=order), torch.randn(2, 3, 4, 4))
  cfg = _cfg(st)
  cfg.device = torch.device('cpu')
  sde = st.sde_lib.get_sde(cfg, None)
  for order in (1, 'rk45'):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      flow.get_flow_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, steps=4, order=order, device='cpu')(None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)(None)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, flow, ref_lib, product_backend):
  product_backend.set_backend(ref_lib)
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(NotImplementedError, match='stk_flow.h'):
    flow.get_flow_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_flow.h'):
    flow.get_flow_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, order='rk45')
  with pytest.raises(NotImplementedError, match='stk_flow.h'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)
  with pytest.raises(NotImplementedError, match='stk_flow.h'):
    flow.flow_sample(_no_model, flow.flow_schedule(4), torch.randn(1, 3, 4, 4))


def test_another_family_and_other_methods_are_refused(st, flow, product_backend):
  cfg = tiny_config(st, 'vp')
  cfg.sampling.method = 'flow'
  with pytest.raises(ValueError, match='RectifiedFlow'):
    st.sampling.get_sampling_fn(cfg, st.sde_lib.get_sde(cfg, None), (2, 3, 8, 8), lambda v: v, 1e-3)
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  for method in ('pc', 'ode', 'dpm_solver', 'adaptive', 'edm', 'consistency', 'parallel'):
    cfg.sampling.method = method
    with pytest.raises(ValueError, match='RectifiedFlow'):
      st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)
  with pytest.raises(ValueError, match='precision'):
    flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, precision='bf16')
  with pytest.raises(ValueError, match='fp16'):
    flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, order='rk45', precision='fp16')
  with pytest.raises(ValueError, match='order'):
    flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, order=3)
  with pytest.raises(ValueError, match='t_end'):
    flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, order='rk45', t_end=1.)
  assert callable(flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, order='rk45'))
  assert callable(flow.get_flow_sampler(_cfg(st), sde, (2, 3, 8, 8), lambda v: v, order=2, precision='fp16'))


def test_get_sampling_fn_dispatches(st, flow, product_backend, monkeypatch):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  monkeypatch.setattr(flow, 'get_flow_sampler', lambda **kw: seen.append(kw) or 'built')
  shape, inv = (2, 3, 8, 8), (lambda v: v)
  keys = ('steps', 'order', 'shift', 'eta', 't_end', 'rtol', 'atol')
  assert st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3) == 'built'
  kw = seen.pop()
  assert tuple(kw[k] for k in keys) == (50, 1, 1., 0., 1e-3, 1e-5, 1e-5)
  assert kw['shape'] == shape and kw['inverse_scaler'] is inv and kw['precision'] == 'fp32' and kw['config'] is cfg and kw['sde'] is sde
  for key in keys:
    del cfg.sampling['flow_' + key]
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  kw = seen.pop()
  assert tuple(kw[k] for k in keys) == (50, 1, 1., 0., 1e-3, 1e-5, 1e-5)
  s = cfg.sampling
  s.flow_steps, s.flow_order, s.flow_shift, s.flow_eta, s.flow_t_end, s.flow_rtol, s.flow_atol = 9, 'rk45', 3., 0.25, 1e-2, 1e-4, 1e-6
  s.precision = 'fp16'
  s.method = 'FLOW'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  kw = seen.pop()
  assert tuple(kw[k] for k in keys) + (kw['precision'],) == (9, 'rk45', 3., 0.25, 1e-2, 1e-4, 1e-6, 'fp16')
