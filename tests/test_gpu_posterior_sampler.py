"""The posterior sampler (posterior_sampling.py) on the device.  Tiny VP and VE networks (16 x 16 images), batch 2, sde.N = 4,
reverse diffusion + Langevin; operators: a 5 x 5 Gaussian blur, a mask, 2 x 2 block averages.

1. measurement_gradient against RefNet on the CPU (torch autograd, the operators restated with conv2d, a product and
   avg_pool2d): g and rnorm within the project's 1e-3 relative bar (BASELINE.json) by rel_err.
2. measurement_gradient with a closed-form linear score on the device against its float64 value, under a bound derived by
   counting roundings through A and A^T (see _analytic_bound); the inputs keep that bound below 1e-4 max|g|.
3. dps_update against the float64 restatement applied to the engine's own score and own vjp, which the test takes itself with
   torch.autograd.grad on the public score function under the same seed.  The guidance increment is held to the 2e-4 the model
   tests hold the engine's arithmetic to (_model_cases.TOL): it goes through some 70 fp32 roundings (about 4e-6) and the
   network's own backward, which answers a seed that differs in its last bits.
4. the sampler loop: bit for bit the loop composed by hand from the public functions; with zeta = 0 bit for bit the unguided
   loop; reproducible; sensitive to y and to denoise; a user callable as operator.
5. refusals.

Worst measured (MI355X): see MEASURED.
"""
import copy

import pytest
import torch

import _posterior_ref as R
import ref_torch
from _model_cases import TOL
from _model_util import rel_err
from _sampler_util import setup, shape_of

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file (38 passed in about 4 s), worst over the VP / VE networks and the three operators:
1. rel_err against RefNet: g 3.4e-7, rnorm 1.1e-7, x0 1.9e-7 (bar 1e-3).
2. the derived bound is at most 7.9e-5 of max|g| (VP, blur); worst error over bound: g 0.058, x0 0.52, rnorm 0.080.
3. rel_err of the guidance increments 1.9e-6, of x and x_mean 6.5e-8, of rnorm 4.7e-8 (bar 2e-4)."""

EPS = 1e-5
U = 2.0 ** -24
SAMPLING = dict(method='pc', predictor='reverse_diffusion', corrector='langevin')
OPERATORS = ['blur', 'mask', 'block_average']
_refs = {}


def _setup(st, lib, family):
  """(cfg, sde, model, ps) of a tiny network; the SDE is a copy with N = 4."""
  cfg, sde, model = setup(st, lib, family, SAMPLING)
  sde = copy.copy(sde)
  sde.N = 4
  return cfg, sde, model, st.posterior_sampling


def _ref(st, cfg, model, family):
  """(cfg_cpu, RefNet) with the model's weights, built once per family."""
  if family not in _refs:
    cfg_cpu = copy.deepcopy(cfg)
    cfg_cpu.device = torch.device('cpu')
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    _refs[family] = (cfg_cpu, st.models.utils.DataParallel(ref_torch.RefNet(cfg_cpu, sd)).eval())
  return _refs[family]


def _mask(seed=2):
  return (torch.rand(1, 1, 16, 16, generator=torch.Generator().manual_seed(seed)) > 0.4).float()


def _operators(ps, name, dev, rounded=True):
  """(the package's operator on the device, its restatement on the host)."""
  if name == 'blur':
    return ps.GaussianBlur(5, 1.0), R.blur(5, 1.0, rounded=rounded)
  if name == 'mask':
    return ps.Masking(_mask().to(dev)), R.masking(_mask())
  return ps.BlockAveraging(2), R.block_average(2)


def _inputs(cfg, A_host, seed=1):
  """A state and a measurement drawn independently of it (so the residual is not dominated by cancellation), on the host."""
  g = torch.Generator().manual_seed(seed)
  shape = shape_of(cfg)
  x = torch.randn(shape, generator=g)
  data = torch.rand(shape, generator=g)
  if cfg.data.centered:
    data = data * 2. - 1.
  return x, A_host(data) + 0.05 * torch.randn(A_host(data).shape, generator=g)


def _coeff(sde, vec_t):
  """(a, s) of sde.marginal_prob at vec_t as fp32 host vectors: the SDE's own values."""
  one = torch.ones((vec_t.shape[0], 1, 1, 1), device=vec_t.device)
  mean, std = sde.marginal_prob(one, vec_t)
  return mean.reshape(-1).float().cpu(), std.float().cpu()


def _f64(t):
  return t.detach().cpu().double()


@pytest.mark.parametrize('name', OPERATORS)
@pytest.mark.parametrize('family', ['vp', 've'])
def test_measurement_gradient_matches_refnet(st, hip_lib, family, name):
  cfg, sde, model, ps = _setup(st, hip_lib, family)
  cfg_cpu, ref = _ref(st, cfg, model, family)
  dev = cfg.device
  A_dev, A_host = _operators(ps, name, dev)
  x, y = _inputs(cfg, A_host)
  t = torch.tensor([0.3, 0.6])
  mu = st.models.utils
  score_fn = mu.get_score_fn(cfg, sde, model, train=False, continuous=True)
  ref_fn = mu.get_score_fn(cfg_cpu, sde, ref, train=False, continuous=True)
  xd = x.to(dev)
  before = xd.clone()
  g, rnorm, x0 = ps.measurement_gradient(score_fn, sde, A_dev, y.to(dev), xd, t.to(dev))
  assert torch.equal(xd, before), 'x was written'
  a, s = _coeff(sde, t)
  want_g, want_rnorm, want_x0 = R.measurement_gradient(lambda xx: ref_fn(xx, t), A_host, y, x, a, s)
  errs = rel_err(g, want_g), rel_err(rnorm, want_rnorm), rel_err(x0, want_x0)
  print(f'measurement_gradient {family} {name}: rel_err g {errs[0]:.3e}, rnorm {errs[1]:.3e}, x0 {errs[2]:.3e}')
  assert max(errs) <= 1e-3, errs
  assert bool(torch.isfinite(g).all()) and g.shape == xd.shape and rnorm.shape == (2,) and float(rnorm.min()) > 0


def _analytic_bound(A, At, depth, x, amu, inv_d, y, a, s):
  """The float64 values of one measurement_gradient with the linear score (amu - x) inv_d, and per-element bounds on what fp32
  may add, in units of u = 2^-24.  A and A^T have non-negative weights, so |A z| <= A |z|; `depth` is the number of terms A sums
  per output (T products and T - 1 sums, held to T + 1 roundings; A^T alike).
    score = (amu - x) inv_d                 2 roundings                       e_s  = 2 u B_s
    x0    = (x + (s s) score) / a           4 of its own                      e_x0 = (s^2 / a) e_s + 5 u B_x0
    m     = A x0                                                              e_m  = A e_x0 + (T + 1) u A B_x0
    r     = y - m                           1                                 e_r  = e_m + 2 u (|y| + A B_x0)
    v     = A^T r                                                             e_v  = A^T e_r + (T + 1) u A^T B_r
    seed  = ((s s) / a) v                   3                                 e_sd = c e_v + 4 u c B_v
    gnet  = -inv_d seed                     1 (torch's backward of the product)   e_gn = inv_d e_sd + 2 u inv_d c B_v
    g     = v / a + gnet                    2                                 e_g  = e_v / a + e_gn + 3 u (B_v / a + inv_d c B_v)
  Returns (g, rnorm, x0, e_g, e_rnorm, e_x0); e_rnorm = |e_r|_2 + 2 u rnorm (the root and the sum)."""
  w = lambda v: R.wide(v, x)
  c = (s * s) / a
  score = (amu - x) * w(inv_d)
  B_s = (amu.abs() + x.abs()) * w(inv_d)
  e_s = 2 * U * B_s
  x0 = (x + w(s * s) * score) / w(a)
  B_x0 = (x.abs() + w(s * s) * B_s) / w(a)
  e_x0 = w(c) * e_s + 5 * U * B_x0
  m = A(x0)
  B_m = A(B_x0)
  e_m = A(e_x0) + (depth + 1) * U * B_m
  r = y - m
  B_r = y.abs() + B_m
  e_r = e_m + 2 * U * B_r
  rnorm = r.reshape(r.shape[0], -1).norm(dim=1)
  e_rnorm = e_r.reshape(r.shape[0], -1).norm(dim=1) + 2 * U * rnorm
  v = At(r)
  B_v = At(B_r)
  e_v = At(e_r) + (depth + 1) * U * B_v
  e_sd = w(c) * e_v + 4 * U * w(c) * B_v
  e_gn = w(inv_d) * e_sd + 2 * U * w(inv_d * c) * B_v
  g = v / w(a) - w(inv_d * c) * v
  e_g = e_v / w(a) + e_gn + 3 * U * (B_v / w(a) + w(inv_d * c) * B_v)
  return g, rnorm, x0, e_g, e_rnorm, e_x0


DEPTH = {'blur': 25, 'mask': 1, 'block_average': 4}
TIMES = {'vp': [0.1, 0.2], 've': [0.25, 0.33]}         # s^2 below a^2 tau^2: v / a and gnet do not cancel


@pytest.mark.parametrize('name', OPERATORS)
@pytest.mark.parametrize('family', ['vp', 've'])
def test_measurement_gradient_matches_closed_form(st, hip_lib, family, name):
  cfg, sde, _, ps = _setup(st, hip_lib, family)
  dev = cfg.device
  A_dev, A_host = _operators(ps, name, dev)
  gen = torch.Generator().manual_seed(7)
  shape = shape_of(cfg)
  t = torch.tensor(TIMES[family])
  a, s = _coeff(sde, t)
  tau = 0.5
  mu = 0.2 * torch.randn(shape[1:], generator=gen)
  # the constants of the score as fp32 tensors, given to both sides: the score is the linear function (amu - x) inv_d exactly
  amu = (R.wide(a, torch.empty(shape)) * mu).float()
  inv_d = (1. / (a.double() ** 2 * tau ** 2 + s.double() ** 2)).float()
  x = (amu + R.wide(torch.sqrt(a * a * tau * tau + s * s), amu) * torch.randn(shape, generator=gen)).float()
  y = A_host(0.3 * torch.randn(shape, generator=gen)).float()
  amu_d, inv_d_d = amu.to(dev), R.wide(inv_d, amu).to(dev)
  score_fn = lambda xx, tt: (amu_d - xx) * inv_d_d
  g, rnorm, x0 = ps.measurement_gradient(score_fn, sde, A_dev, y.to(dev), x.to(dev), t.to(dev))
  d = lambda v: v.double()
  At = R.adjoint(A_host, x)
  want_g, want_rnorm, want_x0, e_g, e_rnorm, e_x0 = _analytic_bound(A_host, At, DEPTH[name], d(x), d(amu), d(inv_d), d(y), d(a),
                                                                      d(s))
  ratio = float(e_g.max() / want_g.abs().max())
  assert ratio < 1e-4, f'the inputs let the bound reach {ratio:.3e} of max|g|'
  err_g, err_x0, err_rn = (_f64(g) - want_g).abs(), (_f64(x0) - want_x0).abs(), (_f64(rnorm) - want_rnorm).abs()
  print(f'closed form {family} {name}: bound {ratio:.3e} of max|g|; worst err / bound: g {float((err_g / e_g.clamp_min(1e-300)).max()):.3f}, '
        f'x0 {float((err_x0 / e_x0).max()):.3f}, rnorm {float((err_rn / e_rnorm).max()):.3f}')
  assert bool((err_x0 <= e_x0).all()) and bool((err_rn <= e_rnorm).all()) and bool((err_g <= e_g).all())


def _predictor(st):
  return st.sampling.get_predictor('reverse_diffusion')


@pytest.mark.parametrize('name', OPERATORS)
@pytest.mark.parametrize('family', ['vp', 've'])
def test_dps_update_matches_restatement(st, hip_lib, family, name):
  cfg, sde, model, ps = _setup(st, hip_lib, family)
  dev = cfg.device
  A_dev, A_host = _operators(ps, name, dev)
  x, y = _inputs(cfg, A_host, seed=3)
  xd, yd = x.to(dev), y.to(dev)
  before = xd.clone()
  t = torch.linspace(sde.T, EPS, sde.N)[1]
  vec_t = torch.ones(2, device=dev) * t
  zeta = 0.8
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  torch.manual_seed(5)
  got, got_mean, got_rnorm = ps.dps_update(cfg, sde, score_fn, _predictor(st), A_dev, yd, xd, t, zeta)
  assert torch.equal(xd, before), 'x was written'
  # by hand under the same seed: the score, then the predictor's own draw, nothing else
  torch.manual_seed(5)
  xg = xd.clone().requires_grad_(True)
  score = score_fn(xg, vec_t)
  with torch.no_grad():
    xp, xpm = _predictor(st)(cfg, sde, lambda xx, tt: score.detach(), False).update_fn(xd, vec_t)
  a, s = _coeff(sde, vec_t)
  a, s = a.double(), s.double()
  x0 = R.tweedie(_f64(xd), _f64(score), a, s)
  r, rnorm = R.residual(_f64(yd), A_host(x0))
  v = R.adjoint(A_host, x0)(r)
  seed = R.seed(v, x0, a, s)
  gnet = torch.autograd.grad(score, xg, seed.float().to(dev))[0]
  want = R.update(_f64(xp), v, _f64(gnet), x0, a, rnorm, zeta)
  want_mean = R.update(_f64(xpm), v, _f64(gnet), x0, a, rnorm, zeta)
  errs = (rel_err(_f64(got) - _f64(xp), want - _f64(xp)), rel_err(_f64(got_mean) - _f64(xpm), want_mean - _f64(xpm)),
          rel_err(got, want), rel_err(got_mean, want_mean), rel_err(got_rnorm, rnorm))
  print(f'dps_update {family} {name}: rel_err of the increments {errs[0]:.3e} {errs[1]:.3e}, of x {errs[2]:.3e}, x_mean '
        f'{errs[3]:.3e}, rnorm {errs[4]:.3e}')
  assert max(errs) <= TOL, errs
  assert float((want - _f64(xp)).abs().max()) > 1e-3, 'the guidance moved nothing'
  # the draw order: zeta = 0 gives the predictor's own outputs bit for bit
  torch.manual_seed(5)
  plain, plain_mean, _ = ps.dps_update(cfg, sde, score_fn, _predictor(st), A_dev, yd, xd, t, 0.0)
  assert torch.equal(plain, xp) and torch.equal(plain_mean, xpm)
  assert not torch.equal(got, xp) and not torch.equal(got, got_mean)
  # a clamp that binds changes the step; the identity predictor returns the guided state itself
  torch.manual_seed(5)
  clipped, _, _ = ps.dps_update(cfg, sde, score_fn, _predictor(st), A_dev, yd, xd, t, zeta, clip=(-0.5, 0.5))
  assert bool(torch.isfinite(clipped).all()) and not torch.equal(clipped, got)
  same, same_mean, _ = ps.dps_update(cfg, sde, score_fn, None, A_dev, yd, xd, vec_t, zeta)
  assert torch.equal(same, same_mean) and torch.equal(xd, before) and not torch.equal(same, xd)


def _sampler_args(st, cfg, sde, operator, **kw):
  S = st.sampling
  args = dict(operator=operator, predictor=_predictor(st), corrector=S.get_corrector('langevin'),
              inverse_scaler=st.datasets.get_data_inverse_scaler(cfg), snr=cfg.sampling.snr, n_steps=1, probability_flow=False,
              continuous=cfg.training.continuous, denoise=True, eps=EPS, zeta=0.5)
  args.update(kw)
  return args


def _by_hand(st, cfg, sde, model, operator, y, seed, zeta):
  """The loop out of the public functions: from the prior, the unguided corrector then the guided predictor over
  linspace(T, eps, N); zeta = None: the unguided predictor (shared_predictor_update_fn) instead."""
  S, ps = st.sampling, st.posterior_sampling
  cont = cfg.training.continuous
  torch.manual_seed(seed)
  with torch.no_grad():
    score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cont)
    x = sde.prior_sampling(shape_of(cfg)).to(y.device)
    timesteps = torch.linspace(sde.T, EPS, sde.N)
    for i in range(sde.N):
      vec_t = torch.ones(2, device=y.device) * timesteps[i]
      x, x_mean = S.shared_corrector_update_fn(x, vec_t, sde, model, S.get_corrector('langevin'), cont, cfg.sampling.snr, 1, cfg)
      if zeta is None:
        x, x_mean = S.shared_predictor_update_fn(x, vec_t, sde, model, _predictor(st), False, cont, cfg)
      else:
        x, x_mean, _ = ps.dps_update(cfg, sde, score_fn, _predictor(st), operator, y, x, vec_t, zeta)
  return st.datasets.get_data_inverse_scaler(cfg)(x_mean)


@pytest.mark.parametrize('name', OPERATORS)
@pytest.mark.parametrize('family', ['vp', 've'])
def test_sampler_loop(st, hip_lib, family, name):
  cfg, sde, model, ps = _setup(st, hip_lib, family)
  dev = cfg.device
  A_dev, A_host = _operators(ps, name, dev)
  _, y = _inputs(cfg, A_host, seed=3)
  y = y.to(dev)
  sampler = ps.get_dps_sampler(cfg, sde, **_sampler_args(st, cfg, sde, A_dev))
  torch.manual_seed(11)
  out = sampler(model, y)
  torch.manual_seed(11)
  again = sampler(model, y)
  assert out.shape == shape_of(cfg) and bool(torch.isfinite(out).all())
  assert torch.equal(out, again), 'two runs under one seed differ'
  assert torch.equal(out, _by_hand(st, cfg, sde, model, A_dev, y, 11, 0.5)), \
      'the loop is not corrector-then-guided-predictor over linspace(T, eps, N) from the prior'
  # zeta = 0: the unguided predictor-corrector loop, bit for bit
  unguided = ps.get_dps_sampler(cfg, sde, **_sampler_args(st, cfg, sde, A_dev, zeta=0.0))
  torch.manual_seed(11)
  plain = unguided(model, y)
  assert torch.equal(plain, _by_hand(st, cfg, sde, model, A_dev, y, 11, None)), 'zeta = 0 is not the unguided loop'
  assert not torch.equal(plain, out)
  # another measurement under the same seed gives another sample; denoise=False returns the noisy state
  _, other = _inputs(cfg, A_host, seed=4)
  torch.manual_seed(11)
  assert not torch.equal(sampler(model, other.to(dev)), out)
  noisy = ps.get_dps_sampler(cfg, sde, **_sampler_args(st, cfg, sde, A_dev, denoise=False))
  torch.manual_seed(11)
  assert not torch.equal(noisy(model, y), out)


def test_user_callable_operator(st, hip_lib):
  cfg, sde, model, ps = _setup(st, hip_lib, 'vp')
  dev = cfg.device
  A = lambda x0: x0.mean(dim=(2, 3))
  y = torch.tensor([[0.3, -0.2, 0.1], [-0.4, 0.0, 0.5]], device=dev)
  sampler = ps.get_dps_sampler(cfg, sde, **_sampler_args(st, cfg, sde, A, clip=(-1., 1.)))
  torch.manual_seed(13)
  out = sampler(model, y)
  torch.manual_seed(13)
  assert out.shape == shape_of(cfg) and bool(torch.isfinite(out).all()) and torch.equal(out, sampler(model, y))
  torch.manual_seed(13)
  assert not torch.equal(sampler(model, -y), out)


def test_refusals(st, hip_lib):
  cfg, sde, model, ps = _setup(st, hip_lib, 'vp')
  dev = cfg.device
  A = ps.BlockAveraging(2)
  x = torch.randn(shape_of(cfg), generator=torch.Generator().manual_seed(1)).to(dev)
  y = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(dev)
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=True)
  args = _sampler_args(st, cfg, sde, A)
  c = copy.deepcopy(cfg)
  c.sampling.precision = 'fp16'
  with pytest.raises(ValueError, match='fp32 only'):
    ps.get_dps_sampler(c, sde, **args)
  sampler = ps.get_dps_sampler(cfg, sde, **args)
  for call in (lambda: sampler(model, y.cpu()), lambda: ps.dps_update(cfg, sde, score_fn, _predictor(st), A, y.cpu(), x, 0.5, 1.),
               lambda: ps.dps_update(cfg, sde, score_fn, _predictor(st), A, y, x.cpu(), 0.5, 1.),
               lambda: ps.measurement_gradient(score_fn, sde, A, y, x.cpu(), 0.5)):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      call()
  # y against the operator's output, on the first step
  for bad in (y[..., :-1].contiguous(), y[:, :2].contiguous(), torch.randn(2, 3, 4, 4, device=dev), y.reshape(2, -1)):
    with pytest.raises(ValueError, match='does not match'):
      sampler(model, bad)
    with pytest.raises(ValueError, match='does not match'):
      ps.measurement_gradient(score_fn, sde, A, bad, x, 0.5)
  for bad in (y.double(), y[:1]):
    with pytest.raises(ValueError):
      ps.dps_update(cfg, sde, score_fn, _predictor(st), A, bad, x, 0.5, 1.)
  for zeta in (-1., float('nan')):
    with pytest.raises(ValueError, match='zeta'):
      ps.dps_update(cfg, sde, score_fn, _predictor(st), A, y, x, 0.5, zeta)
  with pytest.raises(ValueError, match='clip'):
    ps.measurement_gradient(score_fn, sde, A, y, x, 0.5, clip=(1., 1.))

  class Elsewhere(_predictor(st)):
    """asks for the score at another time than the step's"""
    def update_fn(self, x, t, next_t=None):
      return super().update_fn(x, t * 0.5, next_t)

  class Moved(_predictor(st)):
    """asks for the score at another state"""
    def update_fn(self, x, t, next_t=None):
      return super().update_fn(x + 1., t, next_t)

  for predictor in (Elsewhere, Moved):
    with pytest.raises(RuntimeError, match='another point'):
      ps.dps_update(cfg, sde, score_fn, predictor, A, y, x, 0.5, 1.)
  # the state is left usable: a plain step still runs
  out, _, _ = ps.dps_update(cfg, sde, score_fn, _predictor(st), A, y, x, 0.5, 1.)
  assert bool(torch.isfinite(out).all())
