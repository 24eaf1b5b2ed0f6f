"""Host side of dpm_solver.py: the schedule (grid, identities, agreement with the float64 restatement of tests/_dpm_ref.py),
the restatement's own convergence on an analytic Gaussian, the ctypes table of include/stk_solver.h, the refusal of host
tensors and of a library without the header, the dispatch of get_sampling_fn and the argument checks.  No GPU.

Figures of the restatement on the machine that wrote this file (float64, logsnr spacing, steps 20 -> 40 -> 80, the
Gaussian of _dpm_ref.Gaussian((4, 3, 8, 8))): order-1 error ratios 1.94 / 1.97 (VP) and 1.95 / 1.97 (VE); order-2 ratios
3.72 / 3.94 (VP) and 3.78 / 3.95 (VE); order-2 relative error at 40 steps 3.2e-3 (VP) and 2.6e-3 (VE).

The lambda resolution of the fp32 time grid (test_logsnr_spacing_is_uniform): a time t rounds to fp32 within half a unit in
the last place, which moves lambda by at most half of |lambda(t) - lambda(neighbour)| for the farther of its two fp32
neighbours, up to the curvature of lambda over one fp32 spacing (a relative 1e-7: the test allows 1 %).  The restatement
evaluated on the 20-step grids gives a largest such resolution of 2.9e-7 (VP, at t = 0.95), 2.6e-7 (VE, at t = 0.65) and
2.8e-7 (subVP, at t = 0.93), against h = 0.48 / 0.43 / 0.71; a step h_i may differ from the uniform h by the resolutions of
its two ends.  Measured: h deviates by at most 3.8e-7 / 4.8e-7 / 3.4e-7, which is 0.68 / 0.98 / 0.87 of that bound.
"""
import copy
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _dpm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


@pytest.fixture
def dpm(st):
  return st.dpm_solver


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def _families(st):
  S = st.sde_lib
  return {'vp': (S.VPSDE(beta_min=0.1, beta_max=20), R.VP(0.1, 20.)),
          've': (S.VESDE(sigma_min=0.01, sigma_max=50), R.VE(0.01, 50.)),
          'subvp': (S.subVPSDE(beta_min=0.1, beta_max=20), R.SubVP(0.1, 20.))}


def _rel(a, b):
  """Largest element-wise relative difference (an exact zero must be met exactly)."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  assert a.shape == b.shape
  assert np.array_equal(a[b == 0], b[b == 0])
  nz = b != 0
  return float((np.abs(a - b)[nz] / np.abs(b[nz])).max()) if nz.any() else 0.0


def test_module_is_part_of_the_package(st, dpm):
  assert 'dpm_solver' in st.__all__
  assert st._REFERENCE_NAMES['dpm_solver'] is dpm
  for name in ('dpm_schedule', 'dpm_sample', 'get_dpm_sampler'):
    assert callable(getattr(dpm, name)), name


# ---- the schedule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('skip', ['logsnr', 'time', 'time_quadratic'])
@pytest.mark.parametrize('family', ['vp', 've', 'subvp'])
def test_grid(st, dpm, family, skip):
  sde, _ = _families(st)[family]
  for steps in (1, 6, 20):
    s = dpm.dpm_schedule(sde, steps, order=2, skip=skip, eps=EPS)
    assert s.times.dtype == np.float64 and s.times.shape == (steps + 1,) and s.coeffs.shape == (steps, 5)
    assert s.times[0] == float(np.float32(sde.T)) and s.times[-1] == float(np.float32(EPS))
    assert np.array_equal(s.times, s.times.astype(np.float32).astype(np.float64)), 'a time is not fp32-representable'
    assert bool((np.diff(s.times) < 0).all()) and bool((np.diff(s.lam) > 0).all()) and bool((s.h > 0).all())
    assert bool((s.sigma > 0).all())
  # the default ends are the SDE's own
  s = dpm.dpm_schedule(sde, 4)
  assert s.times[0] == 1.0 and s.times[-1] == float(np.float32(getattr(sde, 'eps', 1e-3)))


@pytest.mark.parametrize('family', ['vp', 've', 'subvp'])
def test_logsnr_spacing_is_uniform(st, dpm, family):
  """Uniform in lambda to within the lambda resolution of the fp32 time grid, computed from the restatement on that grid
  (module docstring)."""
  sde, fam = _families(st)[family]
  steps = 20
  s = dpm.dpm_schedule(sde, steps, order=2, skip='logsnr', eps=EPS)
  t32 = s.times.astype(np.float32)
  lam = R.lam_of(fam, s.times)
  res = np.zeros(steps + 1)
  for away in (np.float32(0), np.float32(2)):
    neighbour = np.nextafter(t32, away).astype(np.float64)
    res = np.maximum(res, 0.5 * 1.01 * np.abs(R.lam_of(fam, neighbour) - lam))
  res[0] = res[-1] = 0.                     # the ends are fp32 numbers themselves: nothing was rounded
  uniform = (lam[-1] - lam[0]) / steps
  bound = res[:-1] + res[1:]
  dev = np.abs(np.diff(lam) - uniform)
  floor = 64 * np.finfo(np.float64).eps * np.abs(lam).max()       # float64 evaluation of lambda itself
  print(f'{family}: largest lambda resolution {res.max():.2e} at t = {s.times[res.argmax()]:.4f}; h deviates from uniform by '
        f'at most {dev.max():.2e}, {float((dev / (bound + floor)).max()):.2f} of the bound')
  assert bool((dev <= bound + floor).all())
  assert res.max() < 1e-3 * uniform, 'the bound itself must be far below h, or it says nothing'
  # the package's own lambda is the restatement's
  assert _rel(s.lam, lam) <= 1e-12


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('skip', ['logsnr', 'time', 'time_quadratic'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_consistency_identities(st, dpm, family, skip, order):
  """A sigma_i = sigma_{i+1} and A alpha_i + B = alpha_{i+1}: a constant data prediction is reproduced exactly."""
  sde, _ = _families(st)[family]
  for steps in (6, 20):
    s = dpm.dpm_schedule(sde, steps, order=order, skip=skip, eps=EPS)
    cx, cs, g, A, B = s.coeffs.T
    assert _rel(A * s.sigma[:-1], s.sigma[1:]) <= 1e-12
    assert _rel(A * s.alpha[:-1] + B, s.alpha[1:]) <= 1e-12
    assert _rel(cx * s.alpha[:-1], np.ones(steps)) <= 1e-12 and _rel(cs * s.alpha[:-1], s.sigma[:-1] ** 2) <= 1e-12
    first = [i for i in range(steps) if order == 1 or i == 0 or (steps < 15 and i == steps - 1)]
    assert [i for i in range(steps) if g[i] == 0.] == first and list(np.nonzero(s.orders == 1)[0]) == first
    second = [i for i in range(steps) if i not in first]
    assert _rel(g[second], s.h[second] / (2 * s.h[[i - 1 for i in second]])) <= 1e-12
    assert tuple(s.final[2:]) == (0., 0., 1.) and _rel(s.final[:2], [1 / s.alpha[-1], s.sigma[-1] ** 2 / s.alpha[-1]]) <= 1e-12
  off = dpm.dpm_schedule(sde, 6, order=2, skip=skip, eps=EPS, lower_order_final=False)
  assert list(off.orders) == [1, 2, 2, 2, 2, 2] and bool((off.coeffs[1:, 2] != 0).all())


@pytest.fixture(scope='module')
def convergence():
  """Relative error of the restatement against the exact flow, per family, order and step count: computed once."""
  out = {}
  for name, fam in (('vp', R.VP(0.1, 20.)), ('ve', R.VE(0.01, 50.))):
    gauss = R.Gaussian((4, 3, 8, 8))
    for order in (1, 2):
      out[name, order] = [R.rel(*R.gaussian_run(fam, gauss, steps, order, eps=EPS)) for steps in (20, 40, 80)]
  return out


@pytest.mark.parametrize('family', ['vp', 've'])
def test_restatement_converges_on_a_gaussian(convergence, family):
  """The restatement is proved before anything is compared with it: first order halves its error per doubling of the
  steps, second order quarters it."""
  e1, e2 = convergence[family, 1], convergence[family, 2]
  r1, r2 = [e1[0] / e1[1], e1[1] / e1[2]], [e2[0] / e2[1], e2[1] / e2[2]]
  print(f'{family}: order 1 errors {e1} ratios {r1}; order 2 errors {e2} ratios {r2}')
  assert all(1.8 <= r <= 2.2 for r in r1), r1
  assert all(r >= 3.5 for r in r2), r2
  assert e2[1] <= 1e-2, e2


def test_gaussian_flow_is_the_probability_flow():
  """The closed forms the convergence test leans on: the flow maps the marginal at T to the marginal at t, and its time
  derivative is the probability-flow drift built from the closed-form score (VE: dx/dt = -1/2 d(sigma^2)/dt score)."""
  fam, gauss = R.VE(0.01, 50.), R.Gaussian((2, 3))
  a_T, s_T = fam.alpha_sigma(1.0)
  x_T = gauss.prior(a_T, s_T)
  t, dt = 0.37, 1e-6
  (a0, s0), (a1, s1), (a2, s2) = fam.alpha_sigma(t), fam.alpha_sigma(t + dt), fam.alpha_sigma(t - dt)
  x = gauss.flow(x_T, a_T, s_T, a0, s0)
  slope = (gauss.flow(x_T, a_T, s_T, a1, s1) - gauss.flow(x_T, a_T, s_T, a2, s2)) / (2 * dt)
  drift = -0.5 * (s1 ** 2 - s2 ** 2) / (2 * dt) * gauss.score(x, a0, s0)
  assert R.rel(slope, drift) <= 1e-6


@pytest.mark.parametrize('skip', ['logsnr', 'time', 'time_quadratic'])
@pytest.mark.parametrize('family', ['vp', 've', 'subvp'])
def test_package_schedule_matches_the_restatement(st, dpm, family, skip):
  sde, fam = _families(st)[family]
  for steps, order, lof in ((6, 2, True), (20, 2, True), (6, 1, True), (20, 1, True), (6, 2, False)):
    s = dpm.dpm_schedule(sde, steps, order=order, skip=skip, eps=EPS, lower_order_final=lof)
    r = R.schedule(fam, steps, order=order, skip=skip, eps=EPS, T=1., lower_order_final=lof)
    assert np.array_equal(s.times, r['times'])
    assert list(s.orders) == list(r['orders'])
    worst = max(_rel(s.coeffs, r['coeffs']), _rel(s.final, r['final']), _rel(s.alpha, r['alpha']), _rel(s.sigma, r['sigma']))
    print(f'{family} {skip} steps {steps} order {order}: worst relative difference {worst:.2e}')
    assert worst <= 1e-12
  assert list(dpm.dpm_schedule(sde, 6, eps=EPS).orders) == [1, 2, 2, 2, 2, 1]           # lower_order_final below 15 steps ...
  assert list(dpm.dpm_schedule(sde, 14, eps=EPS).orders)[-1] == 1
  assert list(dpm.dpm_schedule(sde, 15, eps=EPS).orders) == [1] + [2] * 14              # ... and not from 15 on
  assert list(dpm.dpm_schedule(sde, 20, eps=EPS).orders) == [1] + [2] * 19


def test_reciprocal_ve(st, dpm):
  """reciprocal_VESDE's marginal_prob rounds to fp32; the module restates its sigma in float64 from the SDE's constants."""
  sde = st.sde_lib.reciprocal_VESDE()
  s = dpm.dpm_schedule(sde, 10, eps=EPS)
  assert bool((s.alpha == 1).all()) and bool((np.diff(s.lam) > 0).all())
  t = torch.tensor(s.times)
  want = np.sqrt(sde.const * sde.base_sigma ** (2. / s.times) + sde.const_2 * sde.base_sigma_2 ** (2. / s.times))
  assert _rel(s.sigma, want) <= 1e-12
  own = sde.marginal_prob(torch.ones(11, 1, 1, 1), t)[1].double().numpy()
  assert _rel(s.sigma.astype(np.float32).astype(np.float64), own) <= 2e-7       # the SDE's own fp32 value, to fp32 rounding


def test_bad_arguments(st, dpm):
  sde = st.sde_lib.VPSDE()
  with pytest.raises(ValueError, match='order'):
    dpm.dpm_schedule(sde, 10, order=3)
  with pytest.raises(ValueError, match='order'):
    dpm.dpm_schedule(sde, 10, order=0)
  with pytest.raises(ValueError, match='steps'):
    dpm.dpm_schedule(sde, 0)
  with pytest.raises(ValueError, match='steps'):
    dpm.dpm_schedule(sde, 2.5)
  with pytest.raises(ValueError, match='skip'):
    dpm.dpm_schedule(sde, 10, skip='uniform')
  # a grid along which lambda falls: it runs up in time
  with pytest.raises(ValueError, match='VPSDE.*0.5'):
    dpm.dpm_schedule(sde, 10, eps=0.5, T=0.25)

  class Bumpy(st.sde_lib.VESDE):
    """sigma rises, falls and rises again: lambda is not monotone on [eps, T]."""
    def _sigma(self, t):
      return 1. + t + 0.5 * torch.sin(12. * t)

  for skip in ('logsnr', 'time', 'time_quadratic'):
    with pytest.raises(ValueError, match='Bumpy.*lambda.*time'):
      dpm.dpm_schedule(Bumpy(), 10, skip=skip, eps=EPS)

  class Dead(st.sde_lib.VESDE):
    def _sigma(self, t):
      return torch.clamp(t - 0.5, min=0.)

  with pytest.raises(ValueError, match='Dead.*sigma.*time'):
    dpm.dpm_schedule(Dead(), 10, eps=EPS)


# ---- binding and refusals -------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_solver.h declares exactly the entry engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_solver.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_SOLVER
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_dpm_update_f32']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  assert len(table['stk_dpm_update_f32']) == 14
  # the product library exports it; the plain-C checker does not implement this header
  assert 'stk_dpm_update_f32' not in open(os.path.join(ROOT, 'include', 'stk.h')).read()
  assert 'stk_dpm_update_f32' not in open(os.path.join(ROOT, 'oracle', 'stk_ref.c')).read()


def _no_score(x, t):
  raise AssertionError('the score function was evaluated')


def test_host_tensors_are_refused(st, dpm, product_backend, monkeypatch):
  """The package's device error, before anything is computed: no network evaluation, no launch on a host pointer."""
  lib = product_backend.get()
  assert lib.has_solver is True

  def no_launch(*a):
    raise AssertionError('stk_dpm_update_f32 was called on host tensors')

  monkeypatch.setattr(lib, 'dpm_update_f32', no_launch)
  sde = st.sde_lib.VPSDE()
  schedule = dpm.dpm_schedule(sde, 4, eps=EPS)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    dpm.dpm_sample(_no_score, torch.randn(2, 3, 4, 4), schedule)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.device = torch.device('cpu')
  cfg.sampling.method = 'dpm_solver'
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, steps=4, device='cpu')(None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, EPS)(None)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, dpm, ref_lib, product_backend):
  assert ref_lib.has_solver is False
  product_backend.set_backend(ref_lib)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.method = 'dpm_solver'
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(NotImplementedError, match='stk_solver.h'):
    dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_solver.h'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, EPS)
  with pytest.raises(NotImplementedError, match='stk_solver.h'):
    dpm.dpm_sample(_no_score, torch.randn(1, 3, 4, 4), dpm.dpm_schedule(sde, 4, eps=EPS))


def test_get_sampling_fn_dispatches(st, dpm, product_backend, monkeypatch):
  """method = 'dpm_solver' reaches get_dpm_sampler with the config's options (20, 2, 'logsnr', None where absent); the
  other names go where they went."""
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  monkeypatch.setattr(dpm, 'get_dpm_sampler', lambda **kw: seen.append(kw) or 'built')
  cfg.sampling.method = 'dpm_solver'
  shape, inv = (2, 3, 8, 8), (lambda v: v)
  assert st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS) == 'built'
  kw = seen.pop()
  assert (kw['steps'], kw['order'], kw['skip'], kw['clip']) == (20, 2, 'logsnr', None)
  assert kw['eps'] == EPS and kw['shape'] == shape and kw['inverse_scaler'] is inv and kw['precision'] == 'fp32'
  assert kw['denoise'] == cfg.sampling.noise_removal and kw['config'] is cfg and kw['sde'] is sde
  cfg.sampling.dpm_steps, cfg.sampling.dpm_order, cfg.sampling.dpm_skip = 7, 1, 'time'
  cfg.sampling.dpm_clip = (-1., 1.)
  cfg.sampling.precision = 'fp16'
  cfg.sampling.method = 'DPM_Solver'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS)
  kw = seen.pop()
  assert (kw['steps'], kw['order'], kw['skip'], kw['clip'], kw['precision']) == (7, 1, 'time', (-1., 1.), 'fp16')
  cfg.sampling.method = 'dpm'
  with pytest.raises(ValueError, match='Sampler name dpm unknown.'):
    st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS)
  assert not seen


def test_bad_options_fail_when_the_sampler_is_built(st, dpm, product_backend):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.method = 'dpm_solver'
  sde = st.sde_lib.get_sde(cfg, None)
  build = lambda c: st.sampling.get_sampling_fn(c, sde, (2, 3, 8, 8), lambda v: v, EPS)
  assert callable(build(cfg))
  for key, bad, word in (('dpm_order', 3, 'order'), ('dpm_steps', 0, 'steps'), ('dpm_skip', 'log', 'skip'),
                         ('dpm_clip', (1., -1.), 'clip')):
    c = copy.deepcopy(cfg)
    setattr(c.sampling, key, bad)
    with pytest.raises(ValueError, match=word):
      build(c)
  with pytest.raises(ValueError, match='precision'):
    dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, precision='bf16')
