"""The super-resolution sampler (controllable_generation.get_pc_superresolver) on the device: the half-steps against the
float64 restatement applied to the unconditional update's own output, the loop against the half-steps composed by hand, and
the properties of the result.  Tiny VP and VE networks (16 x 16 images), batch 2, sde.N = 4, reverse diffusion + Langevin;
factors 2 and 4, the ones that leave more than one block per side.

Bounds are those of tests/test_gpu_superres.py: k 2^-24 B with k = d + 4, d = 2 and 5 for r = 2 and 4.  The block mean of a
result that went through the config's inverse scaler y = (x + 1) / 2 is held to slope (d + 4) 2^-24 blockmean(B) + 2 2^-24 |y|:
the map is affine and takes at most two fp32 operations, each rounding a value no larger than |y| relative to the result, as
in tests/test_gpu_controllable.py.

Worst measured (MI355X): 2.13 x 2^-24 B over the half-steps; 0.12 of the bound on the block means of a result.
"""
import copy
import functools

import pytest
import torch

import _superres_ref as R
from _model_cases import build_pair, tiny_config
from _stream_util import within

pytestmark = pytest.mark.gpu

EPS = 1e-5
FACTORS = [2, 4]
_built = {}


def _setup(st, lib, family):
  """(cfg, sde, model, cg) of a tiny network, built once per family; sde.N = 4."""
  if family not in _built:
    cfg = tiny_config(st, family)
    cfg.sampling.method, cfg.sampling.predictor, cfg.sampling.corrector = 'pc', 'reverse_diffusion', 'langevin'
    cfg, _, sde, model, _ = build_pair(st, cfg, lib)
    sde.N = 4
    model.eval()
    _built[family] = (cfg, sde, model)
  return _built[family] + (st.controllable_generation,)


def _updates(st, cfg, sde):
  """(predictor, corrector) update functions of the unconditional sampler: update_fn(x, vec_t, model=model)."""
  S = st.sampling
  predict = functools.partial(S.shared_predictor_update_fn, sde=sde, predictor=S.get_predictor('reverse_diffusion'),
                              probability_flow=False, continuous=cfg.training.continuous, config=cfg)
  correct = functools.partial(S.shared_corrector_update_fn, sde=sde, corrector=S.get_corrector('langevin'),
                              continuous=cfg.training.continuous, snr=cfg.sampling.snr, n_steps=1, config=cfg)
  return predict, correct


def _sampler_args(st, cfg, sde, **kw):
  S = st.sampling
  args = dict(predictor=S.get_predictor('reverse_diffusion'), corrector=S.get_corrector('langevin'),
              inverse_scaler=st.datasets.get_data_inverse_scaler(cfg), snr=cfg.sampling.snr, n_steps=1,
              probability_flow=False, continuous=cfg.training.continuous, denoise=True, eps=EPS)
  args.update(kw)
  return args


def _inputs(cfg, cg, r, seed=1):
  """low = the block means of an image in the scaled range of the config, and a state."""
  g = torch.Generator().manual_seed(seed)
  H, C = cfg.data.image_size, cfg.data.num_channels
  data = torch.rand(2, C, H, H, generator=g)
  if cfg.data.centered:
    data = data * 2. - 1.
  x = torch.randn(2, C, H, H, generator=g)
  return cg.block_mean(data.to(cfg.device), r), x.to(cfg.device)


def _coeff(sde, vec_t):
  """(a, s) of sde.marginal_prob at vec_t as float64 CPU vectors: the SDE's own fp32 values."""
  one = torch.ones((vec_t.shape[0], 1, 1, 1), device=vec_t.device)
  mean, std = sde.marginal_prob(one, vec_t)
  return mean.reshape(-1).cpu().double(), std.cpu().double()


def _f64(t):
  return t.detach().cpu().double()


@pytest.mark.parametrize('r', FACTORS)
@pytest.mark.parametrize('which', ['corrector', 'predictor'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_superres_half_step(st, hip_lib, family, which, r):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  predict, correct = _updates(st, cfg, sde)
  update_fn = correct if which == 'corrector' else predict
  low, x = _inputs(cfg, cg, r)
  t = torch.linspace(sde.T, EPS, sde.N)[1]
  x0 = x.clone()
  torch.manual_seed(5)
  got, got_mean = cg.superres_update(update_fn, sde, model, low, r, x, t)
  assert torch.equal(x, x0), 'the half-step wrote into its input'
  # the documented draw order: the update's own noise, then one randn of low's shape on x's device
  torch.manual_seed(5)
  with torch.no_grad():
    vec_t = torch.ones(2, device=cfg.device) * t
    xu, _ = update_fn(x, vec_t, model=model)
    z = torch.randn(low.shape, dtype=torch.float32, device=x.device)
  a, s = _coeff(sde, vec_t)
  if family == 've':
    assert bool((a == 1).all())
  ops = (_f64(xu), _f64(low), _f64(z), a, s, r)
  want, mag = R.restate(*ops), R.magnitude(*ops)
  what = f'superres_update {family} {which} r={r}'
  k = R.DEPTH[r] + 4
  within(got, want[0], mag, k, what + ' x', show=True)
  within(got_mean, want[1], mag, k, what + ' x_mean', show=True)
  assert not torch.equal(got, got_mean) and not torch.equal(got, xu)


def _by_hand(st, cfg, sde, model, low, r, seed):
  """The loop out of the public half-steps: corrector first, then predictor, over linspace(T, eps, N); the initial state is
  the prior moved onto the measurement (a = 1, no noise), written with torch."""
  cg = st.controllable_generation
  predict, correct = _updates(st, cfg, sde)
  H, C = cfg.data.image_size, cfg.data.num_channels
  torch.manual_seed(seed)
  with torch.no_grad():
    x = sde.prior_sampling((low.shape[0], C, H, H)).to(low.device)
    x = x + R.upsample(low - cg.block_mean(x, r), r)
    timesteps = torch.linspace(sde.T, EPS, sde.N)
    for i in range(sde.N):
      x, x_mean = cg.superres_update(correct, sde, model, low, r, x, timesteps[i])
      x, x_mean = cg.superres_update(predict, sde, model, low, r, x, timesteps[i])
  return st.datasets.get_data_inverse_scaler(cfg)(x_mean)


@pytest.mark.parametrize('r', FACTORS)
@pytest.mark.parametrize('family', ['vp', 've'])
def test_superresolver_loop_and_result(st, hip_lib, family, r):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  low, _ = _inputs(cfg, cg, r, seed=3)
  seen = []

  class Recording(st.sampling.get_predictor('reverse_diffusion')):
    """keeps a copy of every predictor output: the last one is the state the final launch started from"""
    def update_fn(self, x, t, next_t=None):
      out = super().update_fn(x, t, next_t)
      seen.append(out[0].clone())
      return out

  superres = cg.get_pc_superresolver(cfg, sde, **_sampler_args(st, cfg, sde), factor=r)
  torch.manual_seed(11)
  out = superres(model, low)
  torch.manual_seed(11)
  again = superres(model, low)
  hand = _by_hand(st, cfg, sde, model, low, r, 11)
  H = cfg.data.image_size
  assert out.shape == (2, cfg.data.num_channels, H, H) and bool(torch.isfinite(out).all())
  assert torch.equal(out, again), 'two runs under one seed differ'
  assert torch.equal(out, hand), 'the loop is not corrector-then-predictor over linspace(T, eps, N) from the moved prior'

  # the result reproduces the measurement: blockmean(out) = inverse_scaler(a_last low).  B of the last launch comes from the
  # last predictor output (the noise does not enter x_mean); its block mean bounds the error of the block mean
  recording = cg.get_pc_superresolver(cfg, sde, **_sampler_args(st, cfg, sde, predictor=Recording), factor=r)
  torch.manual_seed(11)
  assert torch.equal(recording(model, low), out)
  assert len(seen) == sde.N
  inv = (lambda v: (v + 1.) / 2.) if cfg.data.centered else (lambda v: v)
  slope = 0.5 if cfg.data.centered else 1.0
  a, s = _coeff(sde, torch.full((2,), EPS, device=cfg.device))
  want = inv(a[:, None, None, None] * _f64(low))
  mag = R.block_mean(R.magnitude(_f64(seen[-1]), _f64(low), None, a, s, r), r)
  bound = slope * (R.DEPTH[r] + 4) * 2.0 ** -24 * mag + 2 * 2.0 ** -24 * want.abs()
  err = (R.block_mean(_f64(out), r) - want).abs()
  print(f'pc_superresolver {family} r={r}: block means worst err {float(err.max()):.3e}, least bound {float(bound.min()):.3e}, '
        f'worst ratio {float((err / bound).max()):.3f}')
  assert bool((err <= bound).all())
  # ... and the detail was sampled, not copied from the measurement
  assert float((_f64(out) - R.upsample(R.block_mean(_f64(out), r), r)).abs().mean()) > 1e-3, 'no detail was sampled'

  # another measurement under the same seed gives another sample
  other, _ = _inputs(cfg, cg, r, seed=4)
  torch.manual_seed(11)
  assert not torch.equal(superres(model, other), out)
  # denoise=False returns the noisy state
  noisy = cg.get_pc_superresolver(cfg, sde, **_sampler_args(st, cfg, sde, denoise=False), factor=r)
  torch.manual_seed(11)
  assert not torch.equal(noisy(model, low), out)


def test_fp16_superresolution(st, hip_lib):
  """config.sampling.precision = 'fp16' on a net wide enough for the fp16 forms: runs, finite, and reaches the network."""
  cfg = tiny_config(st, 'wide')
  cfg.sampling.method, cfg.sampling.predictor, cfg.sampling.corrector = 'pc', 'reverse_diffusion', 'langevin'
  cfg, _, sde, model, _ = build_pair(st, cfg, hip_lib)
  sde.N = 4
  model.eval()
  cg = st.controllable_generation
  low, _ = _inputs(cfg, cg, 4, seed=6)
  outs = {}
  for precision in ('fp32', 'fp16'):
    c = copy.deepcopy(cfg)
    c.sampling.precision = precision
    torch.manual_seed(17)
    outs[precision] = cg.get_pc_superresolver(c, sde, **_sampler_args(st, c, sde), factor=4)(model, low)
    assert bool(torch.isfinite(outs[precision]).all())
  assert not torch.equal(outs['fp16'], outs['fp32']), 'the fp16 mode did not reach the network'


def test_validation(st, hip_lib):
  cfg, sde, model, cg = _setup(st, hip_lib, 'vp')
  low, x = _inputs(cfg, cg, 4)
  predict, _ = _updates(st, cfg, sde)
  superres = cg.get_pc_superresolver(cfg, sde, **_sampler_args(st, cfg, sde), factor=4)
  for bad in (low.double(), low[0], low[..., :-1].contiguous(), low[:, :2].contiguous(), cg.block_mean(x, 2)):
    with pytest.raises(ValueError):
      superres(model, bad)
  for bad in (low.double(), low[0], low[..., :-1].contiguous(), low[:, :2].contiguous(), low[:1], cg.block_mean(x, 2)):
    with pytest.raises(ValueError):
      cg.superres_update(predict, sde, model, bad, 4, x, 0.5)
  with pytest.raises(ValueError, match='factor'):
    cg.superres_update(predict, sde, model, low, 3, x, 0.5)
  with pytest.raises(ValueError):
    cg.block_mean(x, 3)
  with pytest.raises(ValueError):
    cg.block_mean(x[..., :-1].contiguous(), 2)
  for call in (lambda: superres(model, low.cpu()), lambda: cg.superres_update(predict, sde, model, low.cpu(), 4, x, 0.5),
               lambda: cg.superres_update(predict, sde, model, low, 4, x.cpu(), 0.5), lambda: cg.block_mean(x.cpu(), 4)):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      call()
  # a non-contiguous measurement is taken as it is
  nc = low.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
  assert not nc.is_contiguous()
  torch.manual_seed(2)
  a_, _ = cg.superres_update(predict, sde, model, nc, 4, x, 0.5)
  torch.manual_seed(2)
  b_, _ = cg.superres_update(predict, sde, model, low, 4, x, 0.5)
  assert torch.equal(a_, b_)
