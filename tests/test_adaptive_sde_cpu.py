"""Host side of adaptive_sde.py: the drift / diffusion coefficients against the closed forms of tests/_adaptive_ref.py, the
restatement's own proof that it samples (an analytic Gaussian, many cheap low-dimensional samples), its boundary rules, the
ctypes table of include/stk_adaptive.h, the refusal of host tensors and of a library without the header, and the dispatch of
get_sampling_fn.  No GPU.

The statistical test.  The data are N(mu, s0^2) per element, so the marginal at eps is N(alpha mu, alpha^2 s0^2 + sigma^2)
exactly and the closed-form score makes the reverse SDE exact: what is left is the solver's own discretisation error, which
the tolerances (rtol 0.01, atol 0.0078) keep near 1 % of the spread.  250 samples of 64 elements are drawn, N = 16000 values:
the standard error of their mean is sqrt(var / N) and of their variance var sqrt(2 / (N - 1)) (Gaussian), 0.8 % of the
spread and 1.1 % of the variance; the test allows five of each.  The samples have 64 elements and not fewer because the
algorithm draws fresh noise after a rejection: with a handful of elements E_b is dominated by the sample's own noise, the
accept decision selects on it and the accepted noise is no longer standard normal (at 4 elements the restatement rejects
42 % of its steps and its variance is off by 14 (VP) and 33 (VE) standard errors); the error norm of the published solver
averages over a whole image.  Figures of the restatement on the machine that wrote this file (seed 0, float64): VP mean off
by 1.70 and variance by 1.84 standard errors, 196 iterations at rtol 0.01 and 88 at 0.05, 23 % of the sample-steps rejected;
VE mean off by 0.23 and variance by 1.53 standard errors, 431 iterations and 141, 26 % rejected.
"""
import copy
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _adaptive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3
NAMES = ['stk_sde_commit_f32', 'stk_sde_heun_error_f32', 'stk_sde_stage_f32', 'stk_sde_ws_bytes']


@pytest.fixture
def ada(st):
  return st.adaptive_sde


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
          'subvp': (S.subVPSDE(beta_min=0.1, beta_max=20), R.SubVP(0.1, 20.)),
          've': (S.VESDE(sigma_min=0.01, sigma_max=50), R.VE(0.01, 50.)),
          'rve': (S.reciprocal_VESDE(eta=1e-5, sigma_min=0.01, sigma_max=50), R.RVE(1e-5, 0.01, 50.))}


def test_module_is_part_of_the_package(st, ada):
  assert 'adaptive_sde' in st.__all__
  assert st._REFERENCE_NAMES['adaptive_sde'] is ada
  for name in ('sde_coefficients', 'adaptive_sample', 'get_adaptive_sampler', 'sampling_options'):
    assert callable(getattr(ada, name)), name


# ---- coefficients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['vp', 'subvp', 've', 'rve'])
def test_coefficients_match_the_closed_forms(st, ada, family):
  """float64 in, float64 out, equal to the restatement to float64 rounding: 1e-14 relative is 45 units in the last place,
  room for the two libraries' exp / pow on arguments of magnitude up to 2 / t log(b) and nothing else."""
  sde, fam = _families(st)[family]
  t = np.concatenate([np.linspace(EPS, 1., 41), [0.5 * EPS + 0.37]])
  c, g = ada.sde_coefficients(sde, torch.tensor(t))
  assert c.dtype == torch.float64 and g.dtype == torch.float64 and c.shape == g.shape == (42,)
  want_c, want_g = fam.c(t), fam.g(t)
  assert bool((want_g > 0).all())
  err_c = float(np.abs(c.numpy() - want_c).max() / max(np.abs(want_c).max(), 1e-300))
  err_g = float((np.abs(g.numpy() - want_g) / want_g).max())
  print(f'{family}: c deviates {err_c:.2e}, g deviates {err_g:.2e} (relative)')
  assert err_c <= 1e-14 and err_g <= 1e-14
  # fp32 times give fp32 coefficients: the same functions (sub-VP's 1 - exp(-u) at u = 2e-4 and reciprocal VE's b^(2/t) at
  # t = 1e-3 amplify an fp32 rounding of 6e-8 by up to 1 / u = 5e3, so 1e-3 relative is all that can be asked of them)
  c32, g32 = ada.sde_coefficients(sde, torch.tensor(t, dtype=torch.float32))
  assert c32.dtype == torch.float32 and g32.dtype == torch.float32
  t32 = t.astype(np.float32).astype(np.float64)
  assert float((np.abs(g32.double().numpy() - fam.g(t32)) / fam.g(t32)).max()) <= 1e-3
  assert float(np.abs(c32.double().numpy() - fam.c(t32)).max()) <= 1e-3 * max(np.abs(want_c).max(), 1.)


def test_coefficient_rows(st, ada):
  """The two rows of one iteration, built from sde_coefficients: restated in float64 for VP."""
  sde, fam = _families(st)['vp']
  t, h = np.array([1., 0.6, 0.2]), np.array([0.01, 0.05, 0.199])
  tn = R.next_time(t, h, EPS)
  assert tn[2] == EPS
  a = ada.stage_rows(sde, torch.tensor(t), torch.tensor(h)).numpy()
  b = ada.heun_rows(sde, torch.tensor(tn), torch.tensor(h)).numpy()
  assert np.allclose(a, R.stage_row(fam, t, h), rtol=1e-14, atol=0) and np.allclose(b, R.heun_row(fam, tn, h), rtol=1e-14, atol=0)
  assert np.array_equal(ada.next_time(torch.tensor(t), torch.tensor(h), EPS).numpy(), tn)
  assert a.shape == b.shape == (3, 4) and bool((a[:, 1] == 0).all()) and bool((b[:, 0] == 1).all())


# ---- the restatement is a sampler -------------------------------------------------------------------------------------
MU, S0, N_SAMPLES, DIM = 0.3, 0.5, 250, 64


def _gaussian_run(fam, rtol, dtype=np.float64, seed=0, **kw):
  gauss = R.Gaussian(MU, S0)
  rng = np.random.RandomState(seed)
  a_T, s_T = fam.alpha_sigma(np.float64(1.))
  x = a_T * MU + np.sqrt(gauss.var(a_T, s_T)) * rng.standard_normal((N_SAMPLES, DIM))
  return R.sample(gauss.score_fn(fam, dtype), x, fam, rng.standard_normal, rtol, 0.0078, eps=EPS, dtype=dtype, **kw)


@pytest.fixture(scope='module')
def gaussian_runs():
  return {(name, rtol): _gaussian_run(fam, rtol) for name, fam in (('vp', R.VP(0.1, 20.)), ('ve', R.VE(0.01, 50.)))
          for rtol in (0.01, 0.05)}


@pytest.mark.parametrize('family', ['vp', 've'])
def test_restatement_samples_the_gaussian(gaussian_runs, family):
  fam = R.VP(0.1, 20.) if family == 'vp' else R.VE(0.01, 50.)
  x, iterations, info = gaussian_runs[family, 0.01]
  a, s = fam.alpha_sigma(np.float64(np.float32(EPS)))
  mean, var = a * MU, R.Gaussian(MU, S0).var(a, s)
  n = x.size
  se_mean, se_var = np.sqrt(var / n), var * np.sqrt(2. / (n - 1))
  off_mean, off_var = abs(x.mean() - mean) / se_mean, abs(x.var(ddof=1) - var) / se_var
  loose = gaussian_runs[family, 0.05][1]
  print(f'{family}: mean off by {off_mean:.2f} standard errors, variance by {off_var:.2f}; {iterations} iterations at rtol 0.01, '
        f'{loose} at rtol 0.05; rejected share {info["rejected"].sum() / (info["rejected"].sum() + info["accepted"].sum()):.3f}')
  assert off_mean <= 5. and off_var <= 5.
  assert loose < iterations
  assert bool((info['accepted'] >= 1).all()) and int(info['rejected'].sum()) >= 1, 'the controller never rejected: nothing adaptive ran'


# ---- boundary rules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_boundary_rules(family, dtype):
  fam = R.VP(0.1, 20.) if family == 'vp' else R.VE(0.01, 50.)
  eps = dtype(np.float32(EPS))
  frozen, seen = {}, []

  def watch(i, x, t, h):
    assert bool((t >= eps).all()), 'a sample went below eps'
    done = t <= eps
    assert bool((h[done] == 0).all()) and bool((h[~done] > 0).all())
    for b in np.nonzero(done)[0]:
      if b in frozen:
        assert np.array_equal(frozen[b], x[b]), f'finished sample {b} moved in iteration {i}'
      else:
        frozen[b] = x[b].copy()
    seen.append(int(done.sum()))

  x, iterations, info = _gaussian_run(fam, 0.05, dtype=dtype, watch=watch)
  assert x.dtype == dtype
  assert np.array_equal(info['t'], np.full(N_SAMPLES, eps)), 'a sample did not end at eps exactly'
  assert bool((info['h'] == 0).all())
  assert 0 < len(frozen) < N_SAMPLES + 1 and seen[0] == 0 and max(seen) > 0, 'no sample finished before the last iteration'
  for b, row in frozen.items():
    assert np.array_equal(row, x[b])
  assert bool((info['accepted'] + info['rejected'] <= iterations).all()) and int((info['accepted'] + info['rejected']).max()) == iterations
  with pytest.raises(RuntimeError, match='3 iterations'):
    _gaussian_run(fam, 0.05, dtype=dtype, max_iters=3)


def test_controller_rules():
  """One call on hand-made cases: accepted, rejected, clamped and accepted, finished, non-finite."""
  eps = np.float32(EPS)
  t = np.array([0.5, 0.5, 0.011, eps, 0.5, 0.5], dtype=np.float32)
  h = np.array([0.1, 0.1, np.float32(0.011) - eps, 0., 0.1, 0.1], dtype=np.float32)
  E = np.array([0.5, 2., 0.5, 0., np.nan, np.inf], dtype=np.float32)
  accept, tn, hn = R.controller(t, h, E, eps, 0.9, 0.9)
  assert list(accept) == [True, False, True, False, False, False]
  assert tn[0] == np.float32(0.5) - np.float32(0.1) and tn[1] == t[1] and tn[2] == eps and tn[3] == eps and tn[4] == t[4]
  assert hn[2] == 0 and hn[3] == 0
  assert hn[0] == np.float32(0.9 * float(h[0]) * 0.5 ** -0.9) and hn[1] == np.float32(0.9 * float(h[1]) * 2. ** -0.9)
  assert hn[4] == hn[5] == np.float32(0.9 * float(h[4]) * 0.5)
  # a growing step is clamped to what is left
  _, tn, hn = R.controller(np.array([0.02], dtype=np.float32), np.array([0.01], dtype=np.float32), np.array([1e-3], dtype=np.float32), eps, 0.9, 0.9)
  assert hn[0] == tn[0] - eps


# ---- binding and refusals -------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_adaptive.h declares exactly the entries engine/lib.py binds, argument for argument; the other tables keep
  theirs."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_adaptive.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_ADAPTIVE
  assert sorted(n for n, _ in decls) == sorted(table) == NAMES
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84 and list(L.SIGNATURES_SOLVER) == ['stk_dpm_update_f32']
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  assert re.search(r'\blong\s+stk_sde_ws_bytes\b', text) and L._RESTYPE_ADAPTIVE == {'stk_sde_ws_bytes': L.c_long}
  # the product library exports them; stk.h, the solver's header and the plain-C checker do not know them
  for other in ('include/stk.h', 'include/stk_solver.h', 'oracle/stk_ref.c'):
    body = open(os.path.join(ROOT, *other.split('/'))).read()
    for name in NAMES:
      assert name not in body, (other, name)


def test_workspace_query_is_host_arithmetic(st, product_backend):
  """The query launches nothing, so it answers without a GPU: a positive multiple of 8 B per sample, negative where the
  entries refuse."""
  lib = product_backend.get()
  assert lib.has_adaptive is True
  for B, n in ((1, 1), (3, 105), (2, 192), (16, 3 * 256 * 256), (5000, 7)):
    got = lib.sde_ws_bytes(B, n)
    assert got > 0 and got % (8 * B) == 0, (B, n, got)
    assert got // (8 * B) <= max(1, -(-n // 256)), 'more blocks than a row has work for'
  assert lib.sde_ws_bytes(0, 4) == -1 and lib.sde_ws_bytes(-2, 4) == -1 and lib.sde_ws_bytes(2, 0) == -1
  assert lib.sde_ws_bytes(1, 2 ** 31) == -3 and lib.sde_ws_bytes(2, 2 ** 30) == -3 and lib.sde_ws_bytes(16, 2 ** 40) == -3
  assert lib.sde_ws_bytes(1, 2 ** 31 - 1) > 0


def _no_score(x, t):
  raise AssertionError('the score function was evaluated')


def test_host_tensors_are_refused(st, ada, product_backend, monkeypatch):
  """The package's device error, before anything is computed: no network evaluation, no launch on a host pointer."""
  lib = product_backend.get()

  def no_launch(*a):
    raise AssertionError('an entry of stk_adaptive.h was called on host tensors')

  for name in ('sde_stage_f32', 'sde_heun_error_f32', 'sde_commit_f32', 'sde_ws_bytes'):
    monkeypatch.setattr(lib, name, no_launch)
  sde = st.sde_lib.VPSDE()
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ada.adaptive_sample(_no_score, torch.randn(2, 3, 4, 4), sde)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.device = torch.device('cpu')
  cfg.sampling.method = 'adaptive'
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ada.get_adaptive_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, device='cpu')(None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, EPS)(None)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, ada, ref_lib, product_backend):
  assert ref_lib.has_adaptive is False
  assert not any(hasattr(ref_lib, name[4:]) for name in NAMES)
  product_backend.set_backend(ref_lib)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.method = 'adaptive'
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(NotImplementedError, match='stk_adaptive.h'):
    ada.get_adaptive_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_adaptive.h'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, EPS)
  with pytest.raises(NotImplementedError, match='stk_adaptive.h'):
    ada.adaptive_sample(_no_score, torch.randn(1, 3, 4, 4), sde)


def test_get_sampling_fn_dispatches(st, ada, product_backend, monkeypatch):
  """method = 'adaptive' reaches get_adaptive_sampler with the config's options (the paper's defaults where absent); the
  other names go where they went."""
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  monkeypatch.setattr(ada, 'get_adaptive_sampler', lambda **kw: seen.append(kw) or 'built')
  cfg.sampling.method = 'adaptive'
  shape, inv = (2, 3, 8, 8), (lambda v: v)
  assert st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS) == 'built'
  kw = seen.pop()
  assert cfg.data.centered is True
  assert (kw['rtol'], kw['atol'], kw['h_init'], kw['safety'], kw['exponent']) == (0.01, 0.0078, 0.01, 0.9, 0.9)
  assert kw['eps'] == EPS and kw['shape'] == shape and kw['inverse_scaler'] is inv and kw['precision'] == 'fp32'
  assert kw['denoise'] == cfg.sampling.noise_removal and kw['config'] is cfg and kw['sde'] is sde
  cfg.data.centered = False
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS)
  assert seen.pop()['atol'] == 0.0039
  s = cfg.sampling
  s.adaptive_rtol, s.adaptive_atol, s.adaptive_h_init, s.adaptive_safety, s.adaptive_exponent = 0.05, 0.01, 0.02, 0.8, 0.7
  s.precision = 'fp16'
  s.method = 'Adaptive'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS)
  kw = seen.pop()
  assert (kw['rtol'], kw['atol'], kw['h_init'], kw['safety'], kw['exponent'], kw['precision']) == (0.05, 0.01, 0.02, 0.8, 0.7, 'fp16')
  s.method = 'adaptive_sde'
  with pytest.raises(ValueError, match='Sampler name adaptive_sde unknown.'):
    st.sampling.get_sampling_fn(cfg, sde, shape, inv, EPS)
  assert not seen


def test_bad_options_fail_when_the_sampler_is_built(st, ada, product_backend):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.method = 'adaptive'
  sde = st.sde_lib.get_sde(cfg, None)
  build = lambda c: st.sampling.get_sampling_fn(c, sde, (2, 3, 8, 8), lambda v: v, EPS)
  assert callable(build(cfg))
  for key, bad, word in (('adaptive_rtol', -0.1, 'rtol'), ('adaptive_h_init', 0., 'h_init'), ('adaptive_safety', 0., 'safety'),
                         ('adaptive_exponent', -1., 'exponent')):
    c = copy.deepcopy(cfg)
    setattr(c.sampling, key, bad)
    with pytest.raises(ValueError, match=word):
      build(c)
  with pytest.raises(ValueError, match='precision'):
    ada.get_adaptive_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, precision='bf16')
  with pytest.raises(ValueError, match='max_iters'):
    ada.get_adaptive_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, max_iters=0)
  with pytest.raises(ValueError, match='eps'):
    ada.get_adaptive_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, eps=2.)
