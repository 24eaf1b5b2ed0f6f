"""Host side of the EDM formulation: sde_lib.EDM and its refusals, the score function's conditioning, the schedule of edm.py
against the restatement of tests/_edm_ref.py, the restatement's own second-order convergence on an analytic Gaussian, the
torch-expression loss on the tiny network (checker library) against a float64 restatement of Table 1, the training step, the
ctypes table of include/stk_edm.h, the refusal of host tensors and of a library without the header, and the dispatch of
get_sampling_fn.  No GPU.

Figures of the restatement on the machine that wrote this file (float64, rho = 7, the Gaussian of
_edm_ref.GaussianData((4, 3, 8, 8)), steps 16 -> 32 -> 64 -> 128): relative error against the exact flow 6.4e-2, 1.4e-2,
3.3e-3, 7.8e-4, ratios 4.59 / 4.28 / 4.15.

The loss tolerance.  The loss is compared with a float64 restatement that evaluates Table 1 as the paper writes it, on the
network output F the same tiny network (checker library, fp32) gives at the restatement's own network input, rounded to fp32.
What differs is therefore fp32 rounding alone: of the six coefficients, of x_in (which moves F through the network), and of
the half-dozen element-wise operations behind r.  tests/_tolerances.py states what the other families' loss path is held to
on these f32-operand networks, F32_FWD_RTOL = 7e-6 of the largest entry: the per-sample losses are held to that, relative to
the largest loss of the batch, and the gradient with respect to F relative to its largest entry.  Measured here: 6e-8 / 4.2e-7.
"""
import copy
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _edm_ref as R
from _model_util import build_pair, make_state, patched_rng, tiny_config
from _tolerances import F32_FWD_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


@pytest.fixture
def edm(st):
  return st.edm


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def _cfg(st, family='vp'):
  return st.configs.edm(tiny_config(st, family))


def test_module_is_part_of_the_package(st, edm):
  assert 'edm' in st.__all__ and st._REFERENCE_NAMES['edm'] is edm
  for name in ('edm_schedule', 'edm_sample', 'get_edm_sampler'):
    assert callable(getattr(edm, name)), name


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_edm.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_edm.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_EDM
  assert sorted(n for n, _ in decls) == sorted(table) == sorted(
    ['stk_edm_coeffs_f32', 'stk_edm_ws_bytes', 'stk_edm_loss_f32', 'stk_edm_loss_grad_f32', 'stk_edm_churn_f32', 'stk_edm_step_f32'])
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.has == 'has_edm']
  assert len(row) == 1 and row[0].path == 'include/stk_edm.h' and row[0].table is table
  assert row[0].restype == {'stk_edm_ws_bytes': L.c_long}
  assert [h.has for h in L.OPTIONAL_HEADERS][-2:] == ['has_edm', 'has_guided']
  for name in table:
    assert name not in open(os.path.join(ROOT, 'include', 'stk.h')).read()
    assert name not in open(os.path.join(ROOT, 'oracle', 'stk_ref.c')).read()


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_edm is True and ref_lib.has_edm is False
  assert not hasattr(ref_lib, 'edm_step_f32')


def test_workspace_query_answers_without_a_device(st):
  lib = st.engine.lib.load()
  EINVAL, EUNSUPPORTED = -1, -3
  assert lib.edm_ws_bytes(0, 16) == EINVAL and lib.edm_ws_bytes(-3, 16) == EINVAL and lib.edm_ws_bytes(2, 0) == EINVAL
  assert lib.edm_ws_bytes(2, 2 ** 30) == EUNSUPPORTED and lib.edm_ws_bytes(1, 2 ** 31) == EUNSUPPORTED
  assert lib.edm_ws_bytes(2 ** 20, 2 ** 11) == EUNSUPPORTED
  assert lib.edm_ws_bytes(1, 2 ** 31 - 4) > 0
  # one float64 per (sample, block): 12 blocks share a CIFAR-10 row at batch 128, one block a row of 4
  assert lib.edm_ws_bytes(128, 3072) == 128 * 12 * 8 and lib.edm_ws_bytes(3000, 4) == 3000 * 8
  assert lib.edm_ws_bytes(1, 1) == 8 and lib.edm_ws_bytes(4, 3 * 256 * 256) % 8 == 0


# ---- the family -------------------------------------------------------------------------------------------------------
def test_get_sde_defaults_and_values(st):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.training.sde = 'edm'
  for key in ('sigma_min', 'sigma_max'):
    del cfg.model[key]
  sde = st.sde_lib.get_sde(cfg, None)
  assert isinstance(sde, st.sde_lib.EDM)
  assert (sde.sigma_min, sde.sigma_max, sde.sigma_data, sde.N) == (0.002, 80, 0.5, 1000)
  assert sde.T == 80 and sde.eps == 0.002 and sde.get_t_min(cfg) == 0.002
  cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.sigma_data = 0.01, 50., 1.
  sde = st.sde_lib.get_sde(cfg, None)
  assert (sde.sigma_min, sde.sigma_max, sde.sigma_data) == (0.01, 50., 1.)
  x = torch.randn(3, 2, 4, 4, generator=torch.Generator().manual_seed(0))
  t = torch.tensor([0.5, 2., 50.], dtype=torch.float64)
  mean, std = sde.marginal_prob(x.double(), t)
  assert mean.dtype == std.dtype == torch.float64 and torch.equal(std, t) and torch.equal(mean, x.double())
  drift, g = sde.sde(x, t.float())
  assert not drift.any() and torch.equal(g, torch.sqrt(2. * t.float()))
  torch.manual_seed(1)
  z = sde.prior_sampling((2, 3, 4, 4))
  torch.manual_seed(1)
  assert torch.equal(z, torch.randn(2, 3, 4, 4) * 50.)
  want = -48 / 2. * np.log(2 * np.pi * 50. ** 2) - (z.double() ** 2).sum(dim=(1, 2, 3)) / (2 * 50. ** 2)
  assert torch.allclose(sde.prior_logp(z).double(), want, rtol=1e-6)
  for bad in (dict(sigma_min=0.), dict(sigma_min=90.), dict(sigma_data=0.)):
    with pytest.raises(ValueError, match='sigma'):
      st.sde_lib.EDM(**bad)


REFUSALS = [('data', 'centered', False), ('model', 'scale_by_sigma', True), ('training', 'continuous', False)]
TRAINING_REFUSALS = [('training', k, True) for k in ('mixed', 'importance_sampling', 'likelihood_weighting', 'reconstruction_loss')]


@pytest.mark.parametrize('section,key,value', REFUSALS + TRAINING_REFUSALS, ids=lambda v: str(v))
def test_refusals_name_the_key(st, product_backend, section, key, value):
  """Each refusal is a ValueError naming the key, raised when the step function, the loss or the sampler is built."""
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  assert callable(st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg)))
  assert callable(st.edm.get_edm_sampler(cfg, sde, (2, 3, 16, 16), lambda v: v))
  setattr(getattr(cfg, section), key, value)
  with pytest.raises(ValueError, match=key):
    st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  with pytest.raises(ValueError, match=key):
    st.losses.get_edm_loss_fn(cfg, sde, True)
  if section != 'training' or key == 'continuous':
    with pytest.raises(ValueError, match=key):
      st.edm.get_edm_sampler(cfg, sde, (2, 3, 16, 16), lambda v: v)
    with pytest.raises(ValueError, match=key):
      st.sampling.get_sampling_fn(cfg, sde, (2, 3, 16, 16), lambda v: v, 1e-3)
    with pytest.raises(ValueError, match=key):
      st.models.utils.get_score_fn(cfg, sde, None, train=False, continuous=True)


def test_configs_edm(st):
  for name, make in st.configs.BASELINE_CONFIGS.items():
    base = make()
    cfg = st.configs.edm(base)
    assert base.training.sde != 'edm', 'the shipped config was changed in place'
    assert cfg.training.sde == 'edm' and cfg.sampling.method == 'edm' and cfg.sampling.edm_steps == 18
    assert cfg.data.centered is True and cfg.model.scale_by_sigma is False and cfg.training.continuous is True
    assert (cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.sigma_data) == (0.002, 80., 0.5)
    assert (cfg.training.edm_p_mean, cfg.training.edm_p_std) == (-1.2, 1.2)
    st.models.utils.check_edm_config(cfg, training=True)
    assert isinstance(st.sde_lib.get_sde(cfg, None), st.sde_lib.EDM), name


def test_dpm_schedule_accepts_the_family(st):
  """alpha = 1, sigma = t, lambda = -ln t: A = sigma' / sigma, and a constant data prediction is reproduced."""
  sde = st.sde_lib.EDM()
  s = st.dpm_solver.dpm_schedule(sde, 20)
  assert s.times[0] == 80. and s.times[-1] == float(np.float32(0.002))
  assert bool((s.alpha == 1.).all()) and np.array_equal(s.sigma, s.times)
  assert np.allclose(s.lam, -np.log(s.times), rtol=0, atol=1e-12)
  cx, cs, g, A, B = s.coeffs.T
  assert np.allclose(A, s.sigma[1:] / s.sigma[:-1], rtol=1e-12) and np.allclose(A + B, 1., rtol=0, atol=1e-12)
  assert np.allclose(cx, 1.) and np.allclose(cs, s.sigma[:-1] ** 2, rtol=1e-12)


# ---- the schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [2, 5, 18, 64])
def test_schedule_is_the_float64_formula(st, edm, steps):
  sde = st.sde_lib.EDM()
  s = edm.edm_schedule(sde, steps)
  want = R.sigmas(0.002, 80., steps)
  assert s.sigmas.dtype == np.float64 and np.array_equal(s.sigmas, want)
  i = np.arange(steps)
  formula = (80. ** (1 / 7.) + i / (steps - 1) * (0.002 ** (1 / 7.) - 80. ** (1 / 7.))) ** 7.
  assert np.allclose(s.sigmas[:-1], formula, rtol=2 ** -23, atol=0)
  for times in (s.sigmas, s.t_hat):
    assert np.array_equal(times, times.astype(np.float32).astype(np.float64)), 'a time is not fp32-representable'
  assert s.sigmas[0] == 80. and s.sigmas[-2] == float(np.float32(0.002)) and s.sigmas[-1] == 0.
  assert bool((np.diff(s.sigmas) < 0).all())
  assert not s.gamma.any() and np.array_equal(s.t_hat, s.sigmas[:-1]) and not s.c_eps.any()
  assert s.nfe == 2 * steps - 1 and s.launches == 2 * steps
  assert s.euler.shape == (steps, 6) and s.correct.shape == (steps - 1, 6)
  c_in, c_skip, c_out, c_noise, _ = R.table1(s.sigmas[:-1], 0.5)
  assert np.allclose(s.euler[:, 0], c_skip, rtol=1e-14) and np.allclose(s.euler[:, 1], c_out, rtol=1e-14)
  assert np.array_equal(s.euler[:, 2], s.t_hat) and np.array_equal(s.euler[:, 3], s.sigmas[1:] - s.t_hat)
  assert np.allclose(s.euler[:-1, 4], c_in[1:], rtol=1e-14) and np.allclose(s.euler[:, 5], c_noise, rtol=1e-14, atol=1e-15)
  assert np.allclose(s.correct[:, 0], c_skip[1:], rtol=1e-14) and np.allclose(s.correct[:, 1], c_out[1:], rtol=1e-14)
  assert np.array_equal(s.correct[:, 2], s.sigmas[1:-1]) and np.array_equal(s.correct[:, 3], s.euler[:-1, 3])
  assert np.allclose(s.correct[:, 4], c_in[1:], rtol=1e-14) and np.allclose(s.correct[:, 5], c_noise[1:], rtol=1e-14, atol=1e-15)
  assert np.allclose(s.c_in_hat, c_in, rtol=1e-14)


def test_churn_rule(st, edm):
  """gamma_i = min(s_churn / steps, sqrt(2) - 1) inside [s_tmin, s_tmax], both ends included, else 0."""
  sde = st.sde_lib.EDM()
  plain = edm.edm_schedule(sde, 18)
  lo, hi = float(plain.sigmas[12]), float(plain.sigmas[4])
  s = edm.edm_schedule(sde, 18, s_churn=4.5, s_tmin=lo, s_tmax=hi, s_noise=1.007)
  inside = np.arange(18)[4:13]
  assert np.array_equal(np.nonzero(s.gamma)[0], inside) and np.allclose(s.gamma[inside], 0.25)
  g, t_hat, c_eps = R.churn(plain.sigmas, 18, 4.5, lo, hi, 1.007)
  assert np.array_equal(s.gamma, g) and np.array_equal(s.t_hat, t_hat) and np.allclose(s.c_eps, c_eps, rtol=1e-14)
  assert np.array_equal(s.t_hat, R.fp32(plain.sigmas[:-1] * (1 + s.gamma)))
  assert np.array_equal(s.t_hat[inside], s.t_hat[inside].astype(np.float32).astype(np.float64))
  assert s.launches == 2 * 18 + len(inside)
  # one notch outside either end: that level is not churned
  above = float(np.nextafter(np.float32(lo), np.float32(INF)))
  below = float(np.nextafter(np.float32(hi), np.float32(0)))
  assert np.array_equal(np.nonzero(edm.edm_schedule(sde, 18, s_churn=4.5, s_tmin=above, s_tmax=below).gamma)[0], inside[1:-1])
  # the cap
  assert np.allclose(edm.edm_schedule(sde, 18, s_churn=80).gamma, np.sqrt(2.) - 1.)
  assert edm.edm_schedule(sde, 18, s_churn=80).launches == 2 * 18 + 17          # step 0's churn is the first launch anyway
  # the coefficients of a churned step are those of t^, and its h runs from t^
  c_in, c_skip, c_out, c_noise, _ = R.table1(s.t_hat, 0.5)
  assert np.allclose(s.euler[:, 0], c_skip, rtol=1e-14) and np.allclose(s.euler[:, 5], c_noise, rtol=1e-14, atol=1e-15)
  assert np.array_equal(s.euler[:, 3], s.sigmas[1:] - s.t_hat) and np.allclose(s.correct[:, 4], c_in[1:], rtol=1e-14)


def test_bad_options_name_the_option(st, edm):
  sde = st.sde_lib.EDM()
  for steps in (1, 0, 2.5, -3):
    with pytest.raises(ValueError, match='steps'):
      edm.edm_schedule(sde, steps)
  for kw, word in ((dict(rho=0), 'rho'), (dict(rho=-1), 'rho'), (dict(s_churn=-1), 's_churn'), (dict(s_tmin=-1), 's_tmin'),
                   (dict(s_tmin=2, s_tmax=1), 's_tmax'), (dict(s_noise=-0.1), 's_noise'), (dict(s_churn=float('nan')), 's_churn'),
                   (dict(s_tmax=float('nan')), 's_tmax')):
    with pytest.raises(ValueError, match=word):
      edm.edm_schedule(sde, 18, **kw)
  with pytest.raises(ValueError, match='EDM'):
    edm.edm_schedule(st.sde_lib.VESDE(), 18)


# ---- the Heun loop on an analytic Gaussian -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gaussian():
  g = R.GaussianData((4, 3, 8, 8))
  return g, g.prior(80.)


def test_restatement_converges_at_second_order(gaussian):
  """Algorithm 2 restated in numpy float64 reaches the exact final state of the probability flow at second order: the error
  falls by about four per doubling of the steps."""
  g, x_T = gaussian
  exact = g.flow(x_T, 80., 0.)
  errs = [R.rel(R.heun(g.denoise, x_T, R.sigmas(0.002, 80., steps)), exact) for steps in (16, 32, 64, 128)]
  ratios = [a / b for a, b in zip(errs, errs[1:])]
  print(f'errors {errs} ratios {ratios}')
  assert all(3.5 <= r <= 5.0 for r in ratios), ratios
  assert errs[1] <= 2e-2, errs


def test_schedule_rows_drive_algorithm_2(st, edm, gaussian):
  """The launches' lines on the package's rows (the network output F, not the denoiser) are Algorithm 2: deterministic, and
  the stochastic variant with recorded eps."""
  g, x_T = gaussian
  sde = st.sde_lib.EDM()
  F_of = lambda xin, sigma: R.gaussian_F(g, xin, sigma)
  for steps in (2, 18):
    got = R.launch_loop(edm.edm_schedule(sde, steps), F_of, x_T)
    want = R.heun(g.denoise, x_T, R.sigmas(0.002, 80., steps))
    assert R.rel(got, want) <= 1e-12, steps
  rng = np.random.RandomState(5)
  opts = dict(s_churn=40., s_tmin=0.05, s_tmax=50., s_noise=1.003)
  sch = edm.edm_schedule(sde, 18, **opts)
  churned = int((sch.gamma > 0).sum())
  assert 0 < churned < 18
  noise = [rng.standard_normal(x_T.shape) for _ in range(churned)]
  got = R.launch_loop(sch, F_of, x_T, noise=noise)
  want = R.heun(g.denoise, x_T, R.sigmas(0.002, 80., 18), noise=noise, **opts)
  print(f'stochastic, {churned} churned steps: rows against Algorithm 2 {R.rel(got, want):.2e}')
  assert R.rel(got, want) <= 1e-12
  assert R.rel(got, R.launch_loop(edm.edm_schedule(sde, 18), F_of, x_T)) > 1e-3, 'the churn changed nothing'


# ---- the score function and the loss on the tiny network (checker library) --------------------------------------------------
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


@pytest.fixture(scope='module')
def tiny(st, ref_lib):
  out = {}
  for family in ('vp', 've'):                       # positional and fourier conditioning
    cfg, _, sde, model, _ = build_pair(st, _cfg(st, family), ref_lib)
    out[family] = (cfg, sde, model)
  return out


@pytest.mark.parametrize('family', ['vp', 've'])
def test_score_fn_is_the_denoiser(st, tiny, family):
  """score = (D - x) / sigma^2 with D = c_skip x + c_out F(c_in x; c_noise); positional networks are handed c_noise, fourier
  networks exp(c_noise), whose log the forward takes itself."""
  cfg, sde, model = tiny[family]
  tap = _Tap(model)
  g = torch.Generator().manual_seed(2)
  x = torch.randn(3, 3, 16, 16, generator=g) * 3
  sigma = torch.tensor([0.05, 1.7, 40.])
  with torch.no_grad():
    score = st.models.utils.get_score_fn(cfg, sde, tap, train=False, continuous=True)(x, sigma)
    raw = st.models.utils.get_raw_fn(cfg, sde, tap, train=False, continuous=True)[0](tap.seen[0][0], sigma)
  (x_in, cond, F), (_, cond2, F2) = tap.seen
  c_in, c_skip, c_out, c_noise, _ = (torch.from_numpy(v) for v in R.table1(sigma.double().numpy(), 0.5))
  w = lambda v: v[:, None, None, None]
  assert torch.allclose(x_in.double(), w(c_in) * x.double(), rtol=1e-6, atol=0)
  want_cond = torch.exp(c_noise) if cfg.model.embedding_type == 'fourier' else c_noise
  assert torch.allclose(cond.double(), want_cond, rtol=1e-6, atol=1e-7) and torch.equal(cond, cond2)
  assert torch.equal(raw, F) and torch.equal(F, F2)
  D = w(c_skip) * x.double() + w(c_out) * F.double()
  want = (D - x.double()) / w(torch.from_numpy(sigma.double().numpy() ** 2))
  err = float((score.double() - want).abs().max() / want.abs().max())
  assert err <= 1e-5, err


@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_torch_loss_matches_table_1(st, tiny, family, reduce_mean):
  cfg, sde, model = tiny[family]
  cfg = copy.deepcopy(cfg)
  cfg.training.reduce_mean = reduce_mean
  tap = _Tap(model)
  B = 5
  batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(3))
  loss_fn = st.losses.get_edm_loss_fn(cfg, sde, True)
  model.zero_grad()
  with patched_rng(17):
    losses = loss_fn(tap, batch, importance_sampling=None, t_min=None)
  assert losses.shape == (B,) and losses.dtype == torch.float32
  go = torch.randn(B, generator=torch.Generator().manual_seed(4))
  (losses * go).sum().backward()
  x_in, cond, F = tap.seen[0]
  # the draw order: randn(B) for ln sigma first, randn_like(batch) second
  with patched_rng(17):
    sigma = np.exp(-1.2 + 1.2 * torch.randn(B).double().numpy())
    n = torch.randn_like(batch).double().numpy()
  y = batch.double().numpy()
  c_in, c_skip, c_out, c_noise, lam = R.table1(sigma, 0.5)
  w = lambda v: v[:, None, None, None]
  want_in = w(c_in) * (y + w(sigma) * n)
  assert R.rel(x_in.double().numpy(), want_in) <= 1e-6
  want_cond = np.exp(c_noise) if cfg.model.embedding_type == 'fourier' else c_noise
  assert np.allclose(cond.double().numpy(), want_cond, rtol=2e-6, atol=2e-7)
  # the restatement on the network's answer to ITS OWN input
  tap2 = _Tap(model)
  with torch.no_grad():
    F64 = tap2(torch.from_numpy(want_in).float(), torch.from_numpy(want_cond).float()).double()
  Fv = F64.clone().requires_grad_(True)
  sg, yv, nv = torch.from_numpy(sigma), torch.from_numpy(y), torch.from_numpy(n)
  ci, csk, cou, _, lm = (torch.from_numpy(v) for v in (c_in, c_skip, c_out, c_noise, lam))
  r = w(csk) * (yv + w(sg) * nv) + w(cou) * Fv - yv
  total = (r * r).reshape(B, -1)
  want = lm * (total.mean(dim=1) if reduce_mean else total.sum(dim=1))
  assert np.allclose(want.detach().numpy(), R.loss(F64.numpy(), y, n, sigma, 0.5, reduce_mean), rtol=1e-12)
  (want * go.double()).sum().backward()
  e_loss = float((losses.detach().double() - want.detach()).abs().max() / want.detach().abs().max())
  e_grad = float((F.grad.double() - Fv.grad).abs().max() / Fv.grad.abs().max())
  print(f'{family} reduce_mean={reduce_mean}: loss {e_loss:.2e}, dLoss/dF {e_grad:.2e} (bound {F32_FWD_RTOL:.1e})')
  assert e_loss <= F32_FWD_RTOL and e_grad <= F32_FWD_RTOL
  assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in model.parameters()), 'no gradient reached the network'


def test_draw_order_reproduces_under_a_seed(st, tiny):
  cfg, sde, model = tiny['vp']
  batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(3))
  loss_fn = st.losses.get_edm_loss_fn(cfg, sde, False)
  seen = []
  for seed in (5, 5, 6):
    tap = _Tap(model)
    torch.manual_seed(seed)
    with torch.no_grad():
      losses = loss_fn(tap, batch)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    sigma = torch.exp(-1.2 + 1.2 * torch.randn(4))
    n = torch.randn_like(batch)
    assert torch.equal(torch.get_rng_state(), state), 'the loss drew something else as well'
    c_in = 1. / torch.sqrt(sigma.double() ** 2 + 0.25)
    want_in = (c_in[:, None, None, None] * (batch.double() + sigma.double()[:, None, None, None] * n.double()))
    assert R.rel(tap.seen[0][0].double().numpy(), want_in.numpy()) <= 1e-6
    assert torch.allclose(tap.seen[0][1].double(), torch.log(sigma.double()) / 4., rtol=2e-6, atol=2e-7)
    seen.append(losses)
  assert torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


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


def test_host_tensors_are_refused(st, edm, product_backend, monkeypatch):
  lib = product_backend.get()

  def no_launch(*a):
    raise AssertionError('a kernel was launched on host tensors')

  monkeypatch.setattr(lib, 'edm_churn_f32', no_launch)
  monkeypatch.setattr(lib, 'edm_step_f32', no_launch)
  sde = st.sde_lib.EDM()
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    edm.edm_sample(_no_model, edm.edm_schedule(sde, 4), torch.randn(2, 3, 4, 4))
  cfg = _cfg(st)
  cfg.device = torch.device('cpu')
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    edm.get_edm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, steps=4, device='cpu')(None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)(None)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, edm, ref_lib, product_backend):
  product_backend.set_backend(ref_lib)
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(NotImplementedError, match='stk_edm.h'):
    edm.get_edm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_edm.h'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)
  with pytest.raises(NotImplementedError, match='stk_edm.h'):
    edm.edm_sample(_no_model, edm.edm_schedule(sde, 4), torch.randn(1, 3, 4, 4))


def test_another_family_is_refused(st, edm, product_backend):
  cfg = tiny_config(st, 'vp')
  cfg.sampling.method = 'edm'
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(ValueError, match='EDM'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)
  with pytest.raises(ValueError, match='EDM'):
    st.losses.get_edm_loss_fn(_cfg(st), sde, True)
  with pytest.raises(ValueError, match='precision'):
    edm.get_edm_sampler(_cfg(st), st.sde_lib.EDM(), (2, 3, 8, 8), lambda v: v, precision='bf16')


def test_get_sampling_fn_dispatches(st, edm, product_backend, monkeypatch):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  monkeypatch.setattr(edm, 'get_edm_sampler', lambda **kw: seen.append(kw) or 'built')
  shape, inv = (2, 3, 8, 8), (lambda v: v)
  assert st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3) == 'built'
  kw = seen.pop()
  assert (kw['steps'], kw['rho'], kw['s_churn'], kw['s_tmin'], kw['s_tmax'], kw['s_noise']) == (18, 7., 0., 0., INF, 1.)
  assert kw['shape'] == shape and kw['inverse_scaler'] is inv and kw['precision'] == 'fp32' and kw['config'] is cfg and kw['sde'] is sde
  for key in ('edm_steps', 'edm_rho', 'edm_s_churn', 'edm_s_tmin', 'edm_s_tmax', 'edm_s_noise'):
    del cfg.sampling[key]
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  kw = seen.pop()
  assert (kw['steps'], kw['rho'], kw['s_churn'], kw['s_tmin'], kw['s_tmax'], kw['s_noise']) == (18, 7, 0, 0, INF, 1)
  cfg.sampling.edm_steps, cfg.sampling.edm_rho, cfg.sampling.edm_s_churn = 9, 5., 3.
  cfg.sampling.edm_s_tmin, cfg.sampling.edm_s_tmax, cfg.sampling.edm_s_noise = 0.1, 10., 1.01
  cfg.sampling.precision = 'fp16'
  cfg.sampling.method = 'EDM'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  kw = seen.pop()
  assert (kw['steps'], kw['rho'], kw['s_churn'], kw['s_tmin'], kw['s_tmax'], kw['s_noise'], kw['precision']) == \
      (9, 5., 3., 0.1, 10., 1.01, 'fp16')
