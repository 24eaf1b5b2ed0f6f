"""Host side of the posterior sampler (posterior_sampling.py): its names, the ctypes table of include/stk_posterior.h, the
refusal of host tensors and of a library without the header, the argument checks, and the float64 restatement the GPU tests
compare with -- its sign, its 1 / |r| factor and its clamp rule against torch.autograd.grad of the residual norm written as
one expression.  No GPU."""
import math
import os
import re

import pytest
import torch

import _posterior_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def ps(st):
  """Every test of this file is about posterior_sampling, the restatement's included: without the module there is nothing to
  restate."""
  return st.posterior_sampling


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  from importlib import import_module
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def _sampler_args(st, ps):
  S = st.sampling
  return dict(operator=ps.BlockAveraging(2), predictor=S.get_predictor('reverse_diffusion'),
              corrector=S.get_corrector('langevin'), inverse_scaler=lambda v: v, snr=0.16)


def _tiny(st, family='vp'):
  base = st.configs.cifar10_ddpmpp_nll_st() if family == 'vp' else st.configs.celebahq_uncsnpp_st()
  cfg = st.configs.tiny(base)
  cfg.device = torch.device('cpu')
  return cfg, st.sde_lib.get_sde(cfg, None)


def test_names_are_part_of_the_package(st, ps):
  assert 'posterior_sampling' in st.__all__
  for name in ('get_dps_sampler', 'dps_update', 'measurement_gradient', 'GaussianBlur', 'Masking', 'BlockAveraging'):
    assert callable(getattr(ps, name)), name


def test_signature_table_covers_the_header(st):
  """include/stk_posterior.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_posterior.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_POSTERIOR
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_guide_seed_f32', 'stk_guide_update_f32', 'stk_posterior_ws_bytes',
                                                          'stk_residual_f32', 'stk_tweedie_f32']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_posterior.h']
  assert len(row) == 1 and row[0].has == 'has_posterior' and row[0].table is table
  assert row[0].restype == {'stk_posterior_ws_bytes': L.c_long}
  # the long return type of the header's one query
  assert re.search(r'\blong\s+stk_posterior_ws_bytes\b', text)


def test_host_tensors_are_refused(st, ps, product_backend, monkeypatch):
  """The package's device error, before anything is computed: no entry is called on a host pointer."""
  lib = product_backend.get()
  assert lib.has_posterior is True

  def no_launch(*a):
    raise AssertionError('an entry of stk_posterior.h was called on host tensors')

  for name in ('tweedie_f32', 'residual_f32', 'guide_seed_f32', 'guide_update_f32', 'posterior_ws_bytes'):
    monkeypatch.setattr(lib, name, no_launch)
  cfg, sde = _tiny(st)
  x, y = torch.randn(2, 3, 16, 16), torch.randn(2, 3, 8, 8)
  score_fn = lambda xx, tt: -xx
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ps.measurement_gradient(score_fn, sde, ps.BlockAveraging(2), y, x, 0.5)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ps.dps_update(cfg, sde, score_fn, None, ps.BlockAveraging(2), y, x, 0.5, 1.0)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ps.get_dps_sampler(cfg, sde, **_sampler_args(st, ps))(None, y)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, ps, ref_lib, product_backend):
  assert ref_lib.has_posterior is False
  product_backend.set_backend(ref_lib)
  cfg, sde = _tiny(st)
  with pytest.raises(NotImplementedError, match='stk_posterior.h'):
    ps.get_dps_sampler(cfg, sde, **_sampler_args(st, ps))
  x, y = torch.randn(1, 3, 4, 4), torch.randn(1, 3, 2, 2)
  with pytest.raises(NotImplementedError, match='stk_posterior.h'):
    ps.measurement_gradient(lambda xx, tt: -xx, sde, ps.BlockAveraging(2), y, x, 0.5)
  with pytest.raises(NotImplementedError, match='stk_posterior.h'):
    ps.dps_update(cfg, sde, lambda xx, tt: -xx, None, ps.BlockAveraging(2), y, x, 0.5, 1.0)


def test_bad_arguments_raise_value_error(st, ps, product_backend):
  cfg, sde = _tiny(st)
  args = _sampler_args(st, ps)
  # fp16 has no backward: refused when the sampler is built; so is a precision that does not exist
  cfg.sampling.precision = 'fp16'
  with pytest.raises(ValueError, match='fp32 only'):
    ps.get_dps_sampler(cfg, sde, **args)
  cfg.sampling.precision = 'bf16'
  with pytest.raises(ValueError, match='precision'):
    ps.get_dps_sampler(cfg, sde, **args)
  cfg.sampling.precision = 'fp32'
  ps.get_dps_sampler(cfg, sde, **args)
  for zeta in (-1.0, -1e-30, float('nan')):
    with pytest.raises(ValueError, match='zeta'):
      ps.get_dps_sampler(cfg, sde, **args, zeta=zeta)
  for clip in ((1., -1.), (0., 0.), (float('nan'), 1.), (0., float('nan')), (1.,), (0., 1., 2.), 1.0, 'ab', ('a', 'b')):
    with pytest.raises(ValueError, match='clip'):
      ps.get_dps_sampler(cfg, sde, **args, clip=clip)
  ps.get_dps_sampler(cfg, sde, **args, zeta=0.0, clip=(-1., 1.))
  with pytest.raises(ValueError, match='operator'):
    ps.get_dps_sampler(cfg, sde, **dict(args, operator=None))
  # the operators check their own arguments when they are built
  for size in (0, -3, 3.0, '5', None, True):
    with pytest.raises(ValueError, match='size'):
      ps.GaussianBlur(size, 1.0)
  for std in (0., -1., float('nan'), float('inf')):
    with pytest.raises(ValueError, match='std'):
      ps.GaussianBlur(5, std)
  for factor in (0, 1, 3, 32, 2.0, None, True):
    with pytest.raises(ValueError, match='factor'):
      ps.BlockAveraging(factor)
  for mask in (torch.ones(4), torch.ones(2, 2, dtype=torch.float64), [[1., 0.]], torch.ones(1, 1, 1, 2, 2)):
    with pytest.raises(ValueError, match='mask'):
      ps.Masking(mask)


def test_gaussian_taps_are_float64_rounded_once(ps):
  for size, std in ((1, 1.0), (4, 0.8), (5, 1.0), (8, 2.5), (11, 3.0)):
    blur = ps.GaussianBlur(size, std)
    want = R.gaussian_taps(size, std)
    assert blur.taps.dtype == torch.float32 and blur.taps.shape == (size, size)
    assert torch.equal(blur.taps, want.float()), (size, std)
    assert abs(float(want.sum()) - 1.) <= 1e-15
    assert sum(blur.pad) == size - 1          # 'same': the output keeps the input's extent


# ---- the restatement: sign, 1 / |r| and the clamp rule -----------------------------------------------------------------------
SHAPE = (2, 3, 8, 8)          # rows of 192; the blur sums 25 terms, a residual norm at most 192


def _coefficients(st, family, t):
  """(a, s) [N] of the package's own SDE at times t, in float64."""
  _, sde = _tiny(st, family)
  mean, std = sde.marginal_prob(torch.ones((t.shape[0], 1, 1, 1), dtype=torch.float64), t)
  return mean.reshape(-1), std


def _operator(name, generator):
  if name == 'blur':
    return R.blur(5, 1.0)
  if name == 'mask':
    return R.masking((torch.rand((1, 1) + SHAPE[2:], generator=generator) > 0.4).double())
  return R.block_average(2)


@pytest.mark.parametrize('name', ['blur', 'mask', 'block_average'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_restatement_is_the_gradient_of_the_residual_norm(st, family, name):
  """g / |r| = -d|y - A((x + s^2 score(x)) / a)| / dx to 1e-10 relative: both sides float64, sums of at most 768 terms.  The data
  prediction stays far inside the clamp, which is also tried switched off."""
  gen = torch.Generator().manual_seed(3)
  rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
  a, s = _coefficients(st, family, torch.tensor([0.3, 0.7], dtype=torch.float64))
  if family == 've':
    assert bool((a == 1).all())
  mu, tau = 0.2 * rn(*SHAPE[1:]), 0.5
  score_of = R.gaussian_score(mu, tau, a, s)
  A = _operator(name, gen)
  x = R.wide(a, rn(*SHAPE)) * (mu + tau * rn(*SHAPE)) + R.wide(s, rn(*SHAPE)) * rn(*SHAPE)
  y = A(0.3 * rn(*SHAPE))                       # drawn independently of x
  want = R.norm_gradient(score_of, A, y, x, a, s)
  for lo, hi in ((-R.INF, R.INF), (-1e3, 1e3)):
    g, rnorm, x0 = R.measurement_gradient(score_of, A, y, x, a, s, lo, hi)
    assert float(x0.abs().max()) < 1e2
    got = -g / R.wide(rnorm, g)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-10, (family, name, err)
  # the sign and the factor are pinned: the negated, the unnormalised and the squared-norm gradient are far outside that
  for wrong in (-got, got * R.wide(rnorm, g), 2 * got * R.wide(rnorm, g)):
    assert float((wrong - want).abs().max() / want.abs().max()) > 1e-2
  # a guided step moves down the residual norm: xp + (zeta / |r|) g = xp - zeta d|r|/dx
  zeta = 0.37
  out, mean, _ = R.guided_step(score_of, A, y, x, a, s, zeta, x, 2 * x)
  assert float((out - (x - zeta * want)).abs().max()) <= 1e-10 * float(x.abs().max())
  assert float((mean - (2 * x - zeta * want)).abs().max()) <= 1e-10 * float(x.abs().max())


@pytest.mark.parametrize('family', ['vp', 've'])
def test_restatement_clamp_rule(st, family):
  """Elements whose data prediction sits at a bound: torch.clamp's own derivative is 0 there, the Gaussian score's Jacobian is
  diagonal, so those elements of g are exactly 0, and the rest is still the gradient of the norm."""
  gen = torch.Generator().manual_seed(5)
  rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
  a, s = _coefficients(st, family, torch.tensor([0.3, 0.7], dtype=torch.float64))
  mu, tau = 0.2 * rn(*SHAPE[1:]), 0.5
  score_of = R.gaussian_score(mu, tau, a, s)
  A = R.blur(5, 1.0)
  x = R.wide(a, rn(*SHAPE)) * (mu + tau * rn(*SHAPE)) + R.wide(s, rn(*SHAPE)) * rn(*SHAPE)
  y = A(0.3 * rn(*SHAPE))
  lo, hi = -0.15, 0.2
  g, rnorm, x0 = R.measurement_gradient(score_of, A, y, x, a, s, lo, hi)
  at_bound = (x0 == lo) | (x0 == hi)
  assert 0.05 < float(at_bound.double().mean()) < 0.95 and bool((x0 == lo).any()) and bool((x0 == hi).any())
  assert bool((g[at_bound] == 0).all()), 'an element at a clamp bound received a gradient'
  assert bool((g[~at_bound] != 0).all())
  want = R.norm_gradient(score_of, A, y, x, a, s, lo, hi)
  err = float((-g / R.wide(rnorm, g) - want).abs().max() / want.abs().max())
  assert err <= 1e-10, err
  # ... and the seed is 0 there too
  _, _, _, _, v, _ = R.gradient_parts(score_of, A, y, x, a, s, lo, hi)
  assert bool((R.seed(v, x0, a, s, lo, hi)[at_bound] == 0).all()) and bool((v[at_bound] != 0).any())


def test_restatement_step_size():
  rnorm = torch.tensor([2.0, 0.0, math.inf, math.nan, -1.0], dtype=torch.float64)
  c = R.step_size(rnorm, torch.tensor(3.0, dtype=torch.float64))
  assert c.tolist() == [1.5, 0.0, 0.0, 0.0, 0.0]
