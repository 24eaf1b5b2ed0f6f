"""Consistency training and sampling without a device: the host definitions of soft-truncation_amd/consistency.py (levels,
curriculum, index distribution, coefficients, the sampler's schedule), the binding of include/stk_consistency.h, the config
variant with its refusals, and the torch-expression path of losses.get_consistency_loss_fn around a closed-form network,
against the independent float64 restatement of tests/_consistency_ref.py.

The loss bound.  The torch-expression loss evaluates r in fp32 as the header writes it -- x = y + sigma n (2 roundings), c_skip
x (3), + c_out F (4), on both levels, and their difference (5) -- so |r - r64| <= 6 u B_r elementwise with B_r the same
expression on absolute values, u = 2^-24 (the coefficients are float64 expressions rounded once: one more unit, held by the 6).
S = sum r^2 then deviates by at most sum (2 |r| dr + dr^2), the float64 sum itself by inner 2^-53 relative, and the loss is
non-decreasing in S with d loss / d S = lambda / (2 sqrt(S + c^2)); the result is rounded to fp32 once.  The test holds
|loss - want| <= lambda dS / (2 sqrt(S_lo + c^2)) + 2^-23 want, with S_lo = max(S - dS, 0).  The gradient (dloss lambda c_out /
sqrt(S + c^2)) r in float64 autograd on fp32-rounded r: dr per element, the factor by dS / (2 (S_lo + c^2)) relative.
"""
import copy
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _consistency_ref as R
from _model_util import build_pair, make_state, patched_rng, tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2. ** -24
S_DATA, S_MIN, S_MAX = 0.5, 0.002, 80.
E32 = float(np.float32(S_MIN))
NAMES = ['stk_ct_coeffs_f32', 'stk_ct_pair_f32', 'stk_ct_ws_bytes', 'stk_ct_loss_f32', 'stk_ct_loss_grad_f32', 'stk_ct_step_f32']


@pytest.fixture
def ct(st):
  return st.consistency


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def _cfg(st, family='vp', **kw):
  return st.configs.consistency(tiny_config(st, family), **kw)


def test_module_is_part_of_the_package(st, ct):
  assert 'consistency' in st.__all__ and st._REFERENCE_NAMES['consistency'] is ct
  for name in ('ct_levels', 'ct_num_levels', 'ct_index_pmf', 'get_consistency_sampler', 'consistency_sample'):
    assert callable(getattr(ct, name)), name
  assert callable(st.losses.get_consistency_loss_fn) and callable(st.models.utils.get_consistency_fn)


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_consistency.h declares exactly the entries engine/lib.py binds, argument for argument, in one row that
  stands in front of has_edm."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_consistency.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_CONSISTENCY
  assert sorted(n for n, _ in decls) == sorted(table) == sorted(NAMES)
  assert not set(table) & set(L.SIGNATURES)
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.has == 'has_consistency']
  assert len(row) == 1 and row[0].path == 'include/stk_consistency.h' and row[0].table is table
  assert row[0].restype == {'stk_ct_ws_bytes': L.c_long}
  assert [h.has for h in L.OPTIONAL_HEADERS][-3:] == ['has_consistency', 'has_edm', 'has_guided']
  for name in table:
    assert name not in open(os.path.join(ROOT, 'include', 'stk.h')).read()
    assert name not in open(os.path.join(ROOT, 'oracle', 'stk_ref.c')).read()


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_consistency is True and ref_lib.has_consistency is False
  assert not hasattr(ref_lib, 'ct_step_f32')


def test_workspace_query_answers_without_a_device(st):
  lib = st.engine.lib.load()
  EINVAL, EUNSUPPORTED = -1, -3
  assert lib.ct_ws_bytes(0, 16) == EINVAL and lib.ct_ws_bytes(-3, 16) == EINVAL and lib.ct_ws_bytes(2, 0) == EINVAL
  assert lib.ct_ws_bytes(2, 2 ** 30) == EUNSUPPORTED and lib.ct_ws_bytes(1, 2 ** 31) == EUNSUPPORTED
  assert lib.ct_ws_bytes(128, 3072) == 128 * 12 * 8 and lib.ct_ws_bytes(3000, 4) == 3000 * 8 and lib.ct_ws_bytes(1, 1) == 8


# ---- the definitions ----------------------------------------------------------------------------------------------------
def test_curriculum_tables(ct):
  ks = (0, 49999, 50000, 100000, 349999, 350000, 399999)
  assert [ct.ct_num_levels(k, 400000) for k in ks] == [11, 11, 21, 41, 641, 1281, 1281]
  assert [ct.ct_num_levels(k, 8, s0=2, s1=8) for k in range(8)] == [3, 3, 5, 5, 9, 9, 9, 9]
  assert [ct.ct_num_levels(k, 400000) for k in ks] == [R.num_levels(k, 400000) for k in ks]
  assert ct.ct_num_levels(10 ** 9, 400000) == 1281 and ct.ct_num_levels(5, 3) == 321        # K' is at least 1
  for bad in (dict(s0=0), dict(s0=20, s1=10), dict(K=0)):
    with pytest.raises(ValueError):
      ct.ct_num_levels(**{**dict(k=0, K=8, s0=2, s1=8), **bad})


@pytest.mark.parametrize('N', [11, 1281])
def test_levels_and_pmf(st, ct, N):
  sde = st.sde_lib.EDM(S_MIN, S_MAX, S_DATA)
  lv = ct.ct_levels(sde, N)
  assert lv.dtype == np.float64 and lv.shape == (N,)
  assert lv[0] == E32 and lv[-1] == 80. and np.array_equal(lv, lv.astype(np.float32).astype(np.float64))
  assert bool((np.diff(lv.astype(np.float32)) > 0).all()), 'two levels coincide in fp32'
  assert np.array_equal(lv, R.levels(S_MIN, S_MAX, N))
  pmf = ct.ct_index_pmf(lv)
  want, raw_sum = R.index_pmf(lv)
  assert pmf.shape == (N - 1,) and pmf.dtype == np.float64 and abs(pmf.sum() - 1.) <= 1e-12 and bool((pmf > 0).all())
  assert np.allclose(pmf, want, rtol=1e-9, atol=0) and 1.97 < raw_sum < 1.99
  if N == 1281:
    print(f'N = 1281: smallest raw erf difference {pmf.min() * raw_sum:.2e}, smallest fp32 gap {np.diff(lv).min():.2e}')
    assert 3e-5 < pmf.min() * raw_sum < 5e-5 and 3.8e-5 < np.diff(lv).min() < 4.0e-5
  for bad in (1, 2.5, True):
    with pytest.raises(ValueError, match='N'):
      ct.ct_levels(sde, bad)
  with pytest.raises(ValueError, match='EDM'):
    ct.ct_levels(st.sde_lib.VESDE(), 11)
  with pytest.raises(ValueError, match='p_std'):
    ct.ct_index_pmf(lv, p_std=0.)


def test_coefficients_and_the_boundary_condition(st, ct):
  sigma = np.concatenate([[E32, 80.], np.exp(np.linspace(np.log(0.0021), np.log(79.), 61))]).astype(np.float32).astype(np.float64)
  c_in, c_in_sigma, c_skip, c_out, c_noise = ct.ct_coefficients(sigma, S_DATA, E32)
  assert c_skip[0] == 1. and c_out[0] == 0.
  want = R.boundary(sigma, S_DATA, E32)
  for got, ref in zip((c_in, c_skip, c_out, c_noise), want):
    assert np.allclose(got, ref, rtol=1e-14, atol=1e-300)
  assert np.allclose(c_in_sigma, c_in * sigma, rtol=1e-15)
  assert np.array_equal(np.stack([c_in, c_in_sigma, c_skip, c_out, c_noise]), R.level_rows(sigma, S_DATA, E32))
  rows = [v.numpy() for v in st.models.utils.ct_coefficients(torch.from_numpy(sigma), S_DATA, E32)]
  assert np.allclose(np.stack(rows), R.level_rows(sigma, S_DATA, E32), rtol=1e-15, atol=0)


class _Net(torch.nn.Module):
  """A closed-form network F(x_in, cond) = a tanh(x_in) + b cond: anything callable with train() and eval()."""

  def __init__(self):
    super().__init__()
    self.a = torch.nn.Parameter(torch.tensor(0.7))
    self.seen = []

  def forward(self, x, cond):
    out = self.a * torch.tanh(x) + 0.3 * cond[:, None, None, None]
    if out.requires_grad:
      out.retain_grad()
    self.seen.append((x.detach().clone(), cond.detach().clone(), out, torch.is_grad_enabled()))
    return out


def test_f_at_sigma_min_is_the_identity(st):
  """c_skip = 1 and c_out = 0 exactly at sigma = sigma_min: f(x; sigma_min) = x bit for bit, whatever the network says."""
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  f = st.models.utils.get_consistency_fn(cfg, sde, _Net(), train=False)
  x = torch.randn(3, 3, 5, 7, generator=torch.Generator().manual_seed(0)) * 2
  with torch.no_grad():
    assert torch.equal(f(x, torch.full((3,), S_MIN, dtype=torch.float32)), x)
    y = f(x, torch.tensor([0.01, 1., 80.]))
  assert not torch.equal(y, x) and bool(torch.isfinite(y).all())
  with pytest.raises(ValueError, match='EDM'):
    st.models.utils.get_consistency_fn(cfg, st.sde_lib.VESDE(), _Net())


# ---- the config variant and its refusals ------------------------------------------------------------------------------------
def test_configs_consistency(st):
  for name, make in st.configs.BASELINE_CONFIGS.items():
    base = make()
    cfg = st.configs.consistency(base)
    assert base.training.sde != 'edm' and 'consistency' not in base.training, 'the shipped config was changed in place'
    edm = st.configs.edm(base)
    assert cfg.training.sde == 'edm' and cfg.training.consistency is True and cfg.sampling.method == 'consistency'
    assert (cfg.training.ct_p_mean, cfg.training.ct_p_std, cfg.training.ct_s0, cfg.training.ct_s1) == (-1.1, 2.0, 10, 1280)
    assert cfg.training.ct_huber_c == 0.00054 and cfg.sampling.ct_levels == (80.,) and cfg.sampling.ct_clip is True
    assert cfg.model.to_dict() == edm.model.to_dict() and cfg.data.to_dict() == edm.data.to_dict()
    assert 'consistency' not in edm.training
  two = st.configs.consistency(st.configs.cifar10_ddpmpp_nll_st(), levels=(80, 0.821), sigma_max=80.)
  assert two.sampling.ct_levels == (80, 0.821)


BAD_KEYS = [('ct_s0', 0), ('ct_s0', -2), ('ct_s1', 0), ('ct_s0', 2000), ('ct_p_std', 0.), ('ct_p_std', -1.), ('ct_huber_c', 0.),
            ('ct_huber_c', -1e-3)]


@pytest.mark.parametrize('key,value', BAD_KEYS, ids=lambda v: str(v))
def test_refusals_name_the_key(st, key, value):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  assert callable(st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg)))
  setattr(cfg.training, key, value)
  with pytest.raises(ValueError, match=key):
    st.losses.get_consistency_loss_fn(cfg, sde, True)
  with pytest.raises(ValueError, match=key):
    st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))


@pytest.mark.parametrize('section,key,value', [('data', 'centered', False), ('model', 'scale_by_sigma', True),
                                                ('training', 'continuous', False), ('training', 'mixed', True),
                                                ('training', 'likelihood_weighting', True)], ids=lambda v: str(v))
def test_check_edm_config_applies(st, product_backend, section, key, value):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  setattr(getattr(cfg, section), key, value)
  with pytest.raises(ValueError, match=key):
    st.losses.get_consistency_loss_fn(cfg, sde, True)
  if section != 'training' or key == 'continuous':
    with pytest.raises(ValueError, match=key):
      st.consistency.get_consistency_sampler(cfg, sde, (2, 3, 16, 16), lambda v: v)
    with pytest.raises(ValueError, match=key):
      st.sampling.get_sampling_fn(cfg, sde, (2, 3, 16, 16), lambda v: v, 1e-3)


def test_pick_loss_fn_dispatch(st):
  """training.consistency true on sde_lib.EDM selects the consistency loss; absent or false leaves the EDM loss selected; on
  another family the key selects nothing."""
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  picked = st.losses._pick_loss_fn(cfg, sde, True)
  assert isinstance(picked, st.losses.ConsistencyLoss) and callable(picked.set_step)
  cfg.training.consistency = False
  off = st.losses._pick_loss_fn(cfg, sde, True)
  edm_cfg = st.configs.edm(tiny_config(st, 'vp'))
  assert 'consistency' not in edm_cfg.training
  absent = st.losses._pick_loss_fn(edm_cfg, sde, True)
  for fn in (off, absent):
    assert not hasattr(fn, 'set_step') and 'get_edm_loss_fn' in fn.__qualname__
  vp = tiny_config(st, 'vp')
  vp.training.consistency = True
  assert 'get_sde_loss_fn' in st.losses._pick_loss_fn(vp, st.sde_lib.get_sde(vp, None), True).__qualname__
  with pytest.raises(ValueError, match='EDM'):
    st.losses.get_consistency_loss_fn(_cfg(st), st.sde_lib.get_sde(vp, None), True)


def test_set_step_follows_the_curriculum(st):
  cfg = _cfg(st, s0=2, s1=8)
  cfg.training.n_iters = 8
  sde = st.sde_lib.get_sde(cfg, None)
  loss_fn = st.losses.get_consistency_loss_fn(cfg, sde, True)
  assert loss_fn.N == 3
  seen = []
  for k in range(8):
    assert loss_fn.set_step(k) == loss_fn.N
    lv, pmf = loss_fn.tables()
    assert lv.shape == (loss_fn.N,) and pmf.shape == (loss_fn.N - 1,) and np.array_equal(lv, R.levels(S_MIN, S_MAX, loss_fn.N))
    seen.append(loss_fn.N)
  assert seen == [3, 3, 5, 5, 9, 9, 9, 9]
  assert loss_fn.tables(5)[0] is loss_fn.tables(5)[0], 'the tables are not cached per N'
  big = st.configs.consistency(tiny_config(st, 'vp'))
  big.training.n_iters = 400000
  loss_fn = st.losses.get_consistency_loss_fn(big, sde, True)
  assert [loss_fn.set_step(k) for k in (0, 49999, 50000, 350000)] == [11, 11, 21, 1281]


# ---- the torch-expression loss around a closed-form network ------------------------------------------------------------------
def _operands(B=3, shape=(3, 5, 7), seed=0):
  g = torch.Generator().manual_seed(seed)
  batch = torch.rand((B,) + shape, generator=g) * 2 - 1
  hi = torch.tensor([0.0021, 1.7, 80.][:B], dtype=torch.float32)
  lo = torch.tensor([S_MIN, 1.5, 61.][:B], dtype=torch.float32)
  return batch, hi, lo


@pytest.mark.parametrize('reduce_mean', [True, False], ids=['mean', 'sum'])
def test_torch_loss_and_gradient_match_the_float64_restatement(st, reduce_mean):
  cfg = _cfg(st)
  cfg.training.reduce_mean = reduce_mean
  sde = st.sde_lib.get_sde(cfg, None)
  loss_fn = st.losses.get_consistency_loss_fn(cfg, sde, True)
  batch, hi, lo = _operands()
  B, inner = batch.shape[0], batch[0].numel()
  net = _Net()
  with patched_rng(17):
    losses = loss_fn(net, batch, levels=(hi, lo))
  assert losses.shape == (B,) and losses.dtype == torch.float32 and bool((losses >= 0).all())
  go = torch.randn(B, generator=torch.Generator().manual_seed(4))
  (losses * go).sum().backward()
  # the target first and without gradient, the student second with it
  (xin_lo, cond_lo, F_lo, grad_lo), (xin_hi, cond_hi, F_hi, grad_hi) = net.seen
  assert grad_lo is False and grad_hi is True and not F_lo.requires_grad and F_hi.grad is not None
  with patched_rng(17):
    n = torch.randn_like(batch).double().numpy()
  y, h64, l64 = batch.double().numpy(), hi.double().numpy(), lo.double().numpy()
  w = lambda v: v.reshape(B, 1, 1, 1)
  for xin, cond, sg in ((xin_lo, cond_lo, l64), (xin_hi, cond_hi, h64)):
    c_in, _, _, c_noise = R.boundary(sg, S_DATA, E32)
    assert R.rel(xin.double().numpy(), w(c_in) * (y + w(sg) * n)) <= 1e-6
    assert np.allclose(cond.double().numpy(), c_noise, rtol=2e-6, atol=2e-7)
  c = float(np.float32(0.00054 * np.sqrt(inner)))
  Fh, Fl = F_hi.detach().double().numpy(), F_lo.double().numpy()
  want = R.loss_stable(Fh, Fl, y, n, h64, l64, S_DATA, E32, c, reduce_mean)
  naive = R.loss(Fh, Fl, y, n, h64, l64, S_DATA, E32, c, reduce_mean)
  assert np.allclose(want, naive, rtol=1e-9, atol=0), 'the two float64 forms disagree'
  # the bound of the module docstring
  r = R.residual(Fh, Fl, y, n, h64, l64, S_DATA, E32)
  _, ck_h, co_h, _ = R.boundary(h64, S_DATA, E32)
  _, ck_l, co_l, _ = R.boundary(l64, S_DATA, E32)
  mag = (w(ck_h) * (np.abs(y) + w(h64) * np.abs(n)) + w(co_h) * np.abs(Fh) + w(ck_l) * (np.abs(y) + w(l64) * np.abs(n)) + w(co_l) * np.abs(Fl))
  dr = 6 * U * mag
  S = (r * r).reshape(B, -1).sum(axis=1)
  dS = (2 * np.abs(r) * dr + dr * dr).reshape(B, -1).sum(axis=1) + inner * 2. ** -53 * S
  S_lo = np.maximum(S - dS, 0.)
  lam = 1. / (h64 - l64)
  scale = 1. / inner if reduce_mean else 1.
  tol = lam * dS / (2 * np.sqrt(S_lo + c * c)) * scale + 2. ** -23 * want
  got = losses.detach().double().numpy()
  print(f'reduce_mean={reduce_mean}: loss error {np.abs(got - want)} of bound {tol}')
  assert bool((np.abs(got - want) <= tol).all())
  want_g = R.loss_grad(Fh, Fl, y, n, h64, l64, S_DATA, E32, c, reduce_mean, go.double().numpy())
  k = np.abs(go.double().numpy()) * co_h * lam / np.sqrt(S_lo + c * c) * scale
  g_tol = w(k) * (dr + (dS / (2 * (S_lo + c * c)) + 4 * U).reshape(B, 1, 1, 1) * (np.abs(r) + dr))
  g_err = np.abs(F_hi.grad.double().numpy() - want_g)
  print(f'reduce_mean={reduce_mean}: dLoss/dF worst {float((g_err / np.maximum(g_tol, 1e-300)).max()):.3f} of its bound')
  assert bool((g_err <= g_tol).all())
  assert net.a.grad is not None and float(net.a.grad.abs()) > 0, 'no gradient reached the network'


def test_finite_differences_agree_with_the_float64_gradient():
  """The reference gradient itself, against central differences of the reference loss in float64."""
  rng = np.random.RandomState(2)
  B, shape = 3, (3, 5, 7)
  y, n, Fh, Fl = (rng.standard_normal((B,) + shape) for _ in range(4))
  hi, lo = np.array([0.0021, 1.7, 80.]), np.array([E32, 1.5, 61.])
  go = rng.standard_normal(B)
  for reduce_mean in (False, True):
    for c in (0.00054 * np.sqrt(105.), 3.):
      grad = R.loss_grad(Fh, Fl, y, n, hi, lo, S_DATA, E32, c, reduce_mean, go)
      per_sample = lambda F: go * R.loss_stable(F, Fl, y, n, hi, lo, S_DATA, E32, c, reduce_mean)
      for idx in [(0, 0, 0, 0), (1, 2, 4, 6), (2, 1, 3, 2), (1, 0, 2, 5)]:
        step = np.zeros_like(Fh)
        step[idx] = 1e-5
        up, down = per_sample(Fh + step)[idx[0]], per_sample(Fh - step)[idx[0]]
        fd = (up - down) / 2e-5
        # the truncation error of the central difference (third derivative, relative 1e-6 is generous at this step) and
        # its rounding error: the two float64 loss values carry a few hundred units of 2^-53 each (the sum over 105 terms)
        tol = 1e-6 * abs(grad[idx]) + 256 * 2. ** -53 * (abs(up) + abs(down)) / 2e-5
        assert abs(fd - grad[idx]) <= tol, (idx, fd, grad[idx], tol)


def test_draw_order_reproduces_under_a_seed(st):
  """multinomial(pmf, B) for the indices, randn_like(batch) for the one noise, and -- only in training mode on a model that
  uses dropout -- one randint(0, 2^62, (1,)); nothing else."""
  cfg = _cfg(st, s0=2, s1=8)
  cfg.training.n_iters = 8
  sde = st.sde_lib.get_sde(cfg, None)
  batch, _, _ = _operands(B=3)

  class _Drop(_Net):
    def _uses_dropout(self):
      return True

  for net_cls, train, draws_seed in ((_Net, True, False), (_Drop, False, False), (_Drop, True, True)):
    loss_fn = st.losses.get_consistency_loss_fn(cfg, sde, train)
    loss_fn.set_step(4)                                   # N = 9
    lv, pmf = loss_fn.tables()
    outs = []
    for seed in (5, 5, 6):
      net = net_cls()
      torch.manual_seed(seed)
      with torch.no_grad():
        outs.append(loss_fn(net, batch))
      state = torch.get_rng_state()
      torch.manual_seed(seed)
      idx = torch.multinomial(torch.tensor(pmf, dtype=torch.float32), 3, replacement=True)
      n = torch.randn_like(batch)
      if draws_seed:
        torch.randint(0, 2 ** 62, (1,))
      assert torch.equal(torch.get_rng_state(), state), f'{net_cls.__name__} train={train}: the loss drew something else'
      lo, hi = lv[idx.numpy()], lv[idx.numpy() + 1]
      c_in = R.boundary(lo, S_DATA, E32)[0].reshape(3, 1, 1, 1)
      want_in = c_in * (batch.double().numpy() + lo.reshape(3, 1, 1, 1) * n.double().numpy())
      assert R.rel(net.seen[0][0].double().numpy(), want_in) <= 1e-6, 'the target did not see the lower level of the drawn pair'
      assert np.allclose(net.seen[1][1].double().numpy(), np.log(hi) / 4., rtol=2e-6, atol=2e-7)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---- the step on the tiny network (checker library: the torch-expression path) -------------------------------------------------
def test_training_steps_follow_the_curriculum(st, ref_lib):
  base = _cfg(st, s0=2, s1=8)
  base.training.n_iters = 8
  base.optim.warmup = 2
  cfg, _, sde, model, _ = build_pair(st, base, ref_lib)
  state = make_state(st, cfg, model)
  state['optimizer']._backend = ref_lib
  state['ema'].set_backend(ref_lib)
  seen = []
  real = st.losses.ConsistencyLoss.__call__

  def spy(self, *a, **kw):
    seen.append(self.N)
    return real(self, *a, **kw)

  st.losses.ConsistencyLoss.__call__ = spy
  try:
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    before = [p.detach().clone() for p in model.parameters()]
    for i in range(3):
      batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(100 + i))
      with patched_rng(50 + i):
        losses = step_fn(state, batch)
      assert losses.shape == (4,) and bool(torch.isfinite(losses).all()) and bool((losses >= 0).all())
  finally:
    st.losses.ConsistencyLoss.__call__ = real
  assert state['step'] == 3 and seen == [3, 3, 5]
  assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


# ---- the sampler's schedule, refusals and dispatch ----------------------------------------------------------------------------
def test_schedule_rows(st, ct):
  sde = st.sde_lib.EDM(S_MIN, S_MAX, S_DATA)
  one = ct.consistency_schedule(sde)
  assert one.nfe == 1 and list(one.levels) == [80.] and (one.lo, one.hi) == (-1., 1.)
  sch = ct.consistency_schedule(sde, (80, 0.821, 0.05), clip=False)
  assert sch.nfe == 3 and (sch.lo, sch.hi) == (-float('inf'), float('inf'))
  lv = R.fp32([80, 0.821, 0.05])
  assert np.array_equal(sch.levels, lv)
  rows = R.level_rows(lv, S_DATA, E32)
  assert np.array_equal(sch.rows[:, 0], rows[2]) and np.array_equal(sch.rows[:, 1], rows[3]) and np.array_equal(sch.rows[:, 4], rows[4])
  assert np.allclose(sch.rows[:2, 2], np.sqrt(lv[1:] ** 2 - E32 ** 2), rtol=1e-15) and sch.rows[2, 2] == 0.
  assert np.array_equal(sch.rows[:2, 3], rows[0][1:]) and sch.c_in_first == rows[0][0]
  for bad in ((), (0.5, 0.5), (0.5, 0.8), (81.,), (S_MIN,), (1., 0.001), (float('nan'),), 3.):
    with pytest.raises(ValueError, match='levels'):
      ct.consistency_schedule(sde, bad)
  with pytest.raises(ValueError, match='EDM'):
    ct.consistency_schedule(st.sde_lib.VESDE())


def _no_model(x, c):
  raise AssertionError('the network was evaluated')


def test_host_tensors_and_a_library_without_the_header_are_refused(st, ct, ref_lib, product_backend):
  cfg = _cfg(st)
  sde = st.sde_lib.get_sde(cfg, None)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    ct.consistency_sample(_no_model, ct.consistency_schedule(sde), torch.empty(2, 3, 4, 4))
  cfg.device = torch.device('cpu')
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)(None)
  with pytest.raises(ValueError, match='precision'):
    ct.get_consistency_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, precision='bf16')
  product_backend.set_backend(ref_lib)
  with pytest.raises(NotImplementedError, match='stk_consistency.h'):
    ct.get_consistency_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_consistency.h'):
    st.sampling.get_sampling_fn(cfg, sde, (2, 3, 8, 8), lambda v: v, 1e-3)


def test_get_sampling_fn_dispatches(st, ct, product_backend, monkeypatch):
  cfg = _cfg(st, levels=(80, 0.821))
  sde = st.sde_lib.get_sde(cfg, None)
  seen = []
  monkeypatch.setattr(ct, 'get_consistency_sampler', lambda **kw: seen.append(kw) or 'built')
  shape, inv = (2, 3, 8, 8), (lambda v: v)
  assert st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3) == 'built'
  kw = seen.pop()
  assert kw['levels'] == (80, 0.821) and kw['clip'] is True and kw['precision'] == 'fp32'
  assert kw['shape'] == shape and kw['inverse_scaler'] is inv and kw['config'] is cfg and kw['sde'] is sde
  del cfg.sampling['ct_levels'], cfg.sampling['ct_clip']
  cfg.sampling.precision, cfg.sampling.method = 'fp16', 'Consistency'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  kw = seen.pop()
  assert kw['levels'] is None and kw['clip'] is True and kw['precision'] == 'fp16'


def test_dropout_seed_context_is_additive(st, ref_lib):
  """Executor.dropout_seed pins the seed inside the block and restores what was there; outside it nothing changes."""
  cfg, _, sde, model, _ = build_pair(st, st.configs.consistency(tiny_config(st, 'vp', dropout=0.3)), ref_lib)
  ex = model.module.engine()
  assert ex._pinned_seed is None
  with ex.dropout_seed(7):
    assert ex._pinned_seed == 7
    with ex.dropout_seed(9):
      assert ex._pinned_seed == 9
    assert ex._pinned_seed == 7
  assert ex._pinned_seed is None
  for bad in (-1, 2 ** 62):
    with pytest.raises(ValueError, match='seed'):
      with ex.dropout_seed(bad):
        pass
  # a pinned evaluation draws nothing; an unpinned one draws its one randint as before
  x, t = torch.randn(2, 3, 16, 16), torch.tensor([0.1, 0.2])
  model.train()
  torch.manual_seed(3)
  with torch.no_grad(), ex.dropout_seed(5):
    a = model(x, t)
    state = torch.get_rng_state()
    b = model(x, t)
  torch.manual_seed(3)
  assert torch.equal(torch.get_rng_state(), state), 'a pinned evaluation drew from the generator'
  with torch.no_grad():
    c = model(x, t)
  after = torch.get_rng_state()
  torch.manual_seed(3)
  torch.randint(0, 2 ** 62, (1,))
  assert torch.equal(torch.get_rng_state(), after), 'an unpinned evaluation no longer draws its one randint'
  assert torch.equal(a, b) and not torch.equal(a, c)
