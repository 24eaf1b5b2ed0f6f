"""The inpainting and colourisation samplers (controllable_generation.py) on the device: the half-steps against a float64
blend of the unconditional update's own output, the loop against the half-steps composed by hand, and the properties of the
result.  Tiny VP and VE networks, batch 2, sde.N = 4, reverse diffusion + Langevin.

Bounds are those of tests/test_gpu_impute.py: k 2^-24 B with B the blend on absolute values, k = 8 without the colour mix and
32 with it.  A result that went through the config's inverse scaler y = (x + 1) / 2 is held to slope k 2^-24 B + 2 2^-24 |y|:
the map is affine and takes at most two fp32 operations, each rounding a value no larger than |y| relative to the result.
"""
import copy
import functools

import pytest
import torch

from _model_cases import build_pair, tiny_config
from test_gpu_impute import K_MIX, K_PLAIN, magnitude, matrices, restate, within

pytestmark = pytest.mark.gpu

EPS = 1e-5
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


def _inputs(cfg, seed=1):
  """data in the scaled range of the config, a box mask over batch and channels ([1,1,H,W]), a state."""
  g = torch.Generator().manual_seed(seed)
  H, C = cfg.data.image_size, cfg.data.num_channels
  data = torch.rand(2, C, H, H, generator=g)
  if cfg.data.centered:
    data = data * 2. - 1.
  mask = torch.zeros(1, 1, H, H)
  mask[..., : H // 2 + 1, 1:] = 1.               # known: an odd-sized box; unknown: the rest
  x = torch.randn(2, C, H, H, generator=g)
  return data.to(cfg.device), mask.to(cfg.device), x.to(cfg.device)


def _coeff(sde, vec_t):
  """(a, s) of sde.marginal_prob at vec_t as float64 CPU vectors: the SDE's own fp32 values."""
  one = torch.ones((vec_t.shape[0], 1, 1, 1), device=vec_t.device)
  mean, std = sde.marginal_prob(one, vec_t)
  return mean.reshape(-1).cpu().double(), std.cpu().double()


def _f64(t):
  return t.detach().cpu().double()


@pytest.mark.parametrize('which', ['corrector', 'predictor'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_inpaint_half_step(st, hip_lib, family, which):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  predict, correct = _updates(st, cfg, sde)
  update_fn = correct if which == 'corrector' else predict
  data, mask, x = _inputs(cfg)
  t = torch.linspace(sde.T, EPS, sde.N)[1]
  x0 = x.clone()
  torch.manual_seed(5)
  got, got_mean = cg.inpaint_update(update_fn, sde, model, data, mask, x, t)
  assert torch.equal(x, x0), 'the half-step wrote into its input'
  torch.manual_seed(5)
  with torch.no_grad():
    vec_t = torch.ones(2, device=cfg.device) * t
    xu, _ = update_fn(x, vec_t, model=model)
    z = torch.randn_like(xu)
  a, s = _coeff(sde, vec_t)
  if family == 've':
    assert bool((a == 1).all())
  m = mask.cpu().expand(xu.shape)
  assert torch.equal(got.cpu()[m == 0], xu.cpu()[m == 0]), 'the unknown region is not the update\'s output bit for bit'
  ops = (_f64(xu), _f64(data), _f64(z), _f64(mask), a, s)
  want, mag = restate(*ops), magnitude(*ops)
  what = f'inpaint_update {family} {which}'
  within(got, want[0], mag[0], K_PLAIN, what + ' x')
  within(got_mean, want[1], mag[1], K_PLAIN, what + ' x_mean')
  assert not torch.equal(got.cpu()[m == 1], xu.cpu()[m == 1])


@pytest.mark.parametrize('which', ['corrector', 'predictor'])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_colorize_half_step(st, hip_lib, family, which):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  predict, correct = _updates(st, cfg, sde)
  update_fn = correct if which == 'corrector' else predict
  data, _, x = _inputs(cfg, seed=2)
  gray = data.mean(dim=1, keepdim=True).repeat(1, 3, 1, 1).contiguous()
  t = torch.linspace(sde.T, EPS, sde.N)[2]
  torch.manual_seed(7)
  got, got_mean = cg.colorize_update(update_fn, sde, model, gray, x, t)
  torch.manual_seed(7)
  with torch.no_grad():
    vec_t = torch.ones(2, device=cfg.device) * t
    xu, _ = update_fn(x, vec_t, model=model)
    z = torch.randn_like(xu)
  a, s = _coeff(sde, vec_t)
  m64, u64, _, _ = matrices()
  mask = _f64(cg.get_mask(gray[:1]))
  ops = (_f64(xu), _f64(gray), _f64(z), mask, a, s)
  # the kernel's RGB result is within k 2^-24 B_rgb of v inv(M); decoupled again in float64, within that bound times |M|
  want = restate(*ops, mix=m64, unmix=None)
  mag = magnitude(*ops, mix=m64, unmix=u64)
  dec = lambda t64: torch.einsum('bihw,ij->bjhw', t64, m64)
  mag = [torch.einsum('bihw,ij->bjhw', b, m64.abs()) for b in mag]
  what = f'colorize_update {family} {which}'
  within(dec(_f64(got)), want[0], mag[0], K_MIX, what + ' decoupled x')
  within(dec(_f64(got_mean)), want[1], mag[1], K_MIX, what + ' decoupled x_mean')
  # ... and the public transforms agree with the einsum they stand for
  for fn, mat in ((cg.decouple, m64), (cg.couple, u64)):
    y64 = torch.einsum('bihw,ij->bjhw', _f64(got), mat)
    b = torch.einsum('bihw,ij->bjhw', _f64(got).abs(), mat.abs())
    within(fn(got), y64, b, K_MIX, f'{fn.__name__} {family}')


def _by_hand(st, cfg, sde, model, data, mask, seed):
  """upstream's loop out of the public half-steps: corrector first, then predictor, over linspace(T, eps, N)."""
  cg = st.controllable_generation
  predict, correct = _updates(st, cfg, sde)
  torch.manual_seed(seed)
  with torch.no_grad():
    x = data * mask + sde.prior_sampling(data.shape).to(data.device) * (1. - mask)
    timesteps = torch.linspace(sde.T, EPS, sde.N)
    for i in range(sde.N):
      x, x_mean = cg.inpaint_update(correct, sde, model, data, mask, x, timesteps[i])
      x, x_mean = cg.inpaint_update(predict, sde, model, data, mask, x, timesteps[i])
  return st.datasets.get_data_inverse_scaler(cfg)(x_mean)


def _known_region(cfg, sde, got, data, mask, k, what):
  """inverse_scaler(a(eps) data) where the mask is 1, within the scaled blend bound (module docstring)."""
  inv = lambda v: (v + 1.) / 2. if cfg.data.centered else v
  slope = 0.5 if cfg.data.centered else 1.0
  a, _ = _coeff(sde, torch.full((data.shape[0],), EPS, device=data.device))
  mean = a[:, None, None, None] * _f64(data)
  m = mask.cpu().expand(data.shape) == 1
  want = inv(mean)
  bound = slope * k * 2.0 ** -24 * mean.abs() + 2 * 2.0 ** -24 * want.abs()
  err = (_f64(got) - want).abs()
  print(f'{what}: known region worst err {float(err[m].max()):.3e}, bound there {float(bound[m].min()):.3e}')
  assert bool((err[m] <= bound[m]).all()), what
  return want


@pytest.mark.parametrize('family', ['vp', 've'])
def test_inpainter_loop_and_result(st, hip_lib, family):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  data, mask, _ = _inputs(cfg, seed=3)
  inpaint = cg.get_pc_inpainter(cfg, sde, **_sampler_args(st, cfg, sde))
  torch.manual_seed(11)
  out = inpaint(model, data, mask)
  torch.manual_seed(11)
  again = inpaint(model, data, mask)
  hand = _by_hand(st, cfg, sde, model, data, mask, 11)
  assert out.shape == data.shape and bool(torch.isfinite(out).all())
  assert torch.equal(out, again), 'two runs under one seed differ'
  assert torch.equal(out, hand), 'the loop is not corrector-then-predictor over linspace(T, eps, N)'
  want = _known_region(cfg, sde, out, data, mask, K_PLAIN, f'pc_inpainter {family}')
  m = mask.cpu().expand(data.shape) == 1
  if family == 've':
    assert torch.equal(out.cpu()[m], data.cpu()[m])          # a = 1, identity scaler: the data itself
  assert float((_f64(out) - want).abs()[~m].mean()) > 1e-3, 'the unknown region was not sampled'
  # denoise=False returns the noisy state: another tensor, same known mean up to s(eps) z
  noisy = cg.get_pc_inpainter(cfg, sde, **_sampler_args(st, cfg, sde, denoise=False))
  torch.manual_seed(11)
  assert not torch.equal(noisy(model, data, mask), out)


@pytest.mark.parametrize('family', ['vp', 've'])
def test_colorizer_result(st, hip_lib, family):
  cfg, sde, model, cg = _setup(st, hip_lib, family)
  data, _, _ = _inputs(cfg, seed=4)
  gray = data.mean(dim=1, keepdim=True).repeat(1, 3, 1, 1).contiguous()
  seen = []

  class Recording(st.sampling.get_predictor('reverse_diffusion')):
    """keeps a copy of every predictor output: the last one is the state the final blend started from"""
    def update_fn(self, x, t, next_t=None):
      out = super().update_fn(x, t, next_t)
      seen.append(out[0].clone())
      return out

  colorize = cg.get_pc_colorizer(cfg, sde, **_sampler_args(st, cfg, sde, predictor=Recording, inverse_scaler=lambda v: v))
  torch.manual_seed(13)
  out = colorize(model, gray)
  assert len(seen) == sde.N
  xu = seen[-1]
  torch.manual_seed(13)
  assert torch.equal(out, colorize(model, gray))
  assert out.shape == gray.shape and bool(torch.isfinite(out).all())
  # channel 0 of the decoupled result is a(eps) times that of the decoupled gray image.  B of the final x_mean in RGB, from
  # the last predictor output (the noise does not enter it: where the mask is 1 x_mean takes the mean alone); decoupled
  # again in float64 the error is within k 2^-24 B |M|
  m64, u64, _, _ = matrices()
  a, s = _coeff(sde, torch.full((2,), EPS, device=cfg.device))
  dec = lambda t64, mat=m64: torch.einsum('bihw,ij->bjhw', t64, mat)
  ops = (_f64(xu), _f64(gray), None, _f64(cg.get_mask(gray[:1])), a, s)
  want = restate(*ops, mix=m64, unmix=None)[1]
  mag = dec(magnitude(*ops, mix=m64, unmix=u64)[1], m64.abs())
  assert torch.equal(want[:, 0], (a[:, None, None, None] * dec(_f64(gray)))[:, 0])
  within(dec(_f64(out))[:, :1], want[:, :1], mag[:, :1], K_MIX, f'pc_colorizer {family} decoupled channel 0')
  within(dec(_f64(out)), want, mag, K_MIX, f'pc_colorizer {family} decoupled x_mean')
  assert float(dec(_f64(out))[:, 1:].abs().mean()) > 1e-3, 'no colour was sampled'


def test_fp16_inpainting(st, hip_lib):
  """config.sampling.precision = 'fp16' on a net wide enough for the fp16 forms: runs, finite, same known region."""
  cfg = tiny_config(st, 'wide')
  cfg.sampling.method, cfg.sampling.predictor, cfg.sampling.corrector = 'pc', 'reverse_diffusion', 'langevin'
  cfg, _, sde, model, _ = build_pair(st, cfg, hip_lib)
  sde.N = 4
  model.eval()
  cg = st.controllable_generation
  data, mask, _ = _inputs(cfg, seed=6)
  outs = {}
  for precision in ('fp32', 'fp16'):
    c = copy.deepcopy(cfg)
    c.sampling.precision = precision
    torch.manual_seed(17)
    outs[precision] = cg.get_pc_inpainter(c, sde, **_sampler_args(st, c, sde))(model, data, mask)
    assert bool(torch.isfinite(outs[precision]).all())
    _known_region(c, sde, outs[precision], data, mask, K_PLAIN, f'pc_inpainter wide {precision}')
  assert not torch.equal(outs['fp16'], outs['fp32']), 'the fp16 mode did not reach the network'


def test_validation(st, hip_lib):
  cfg, sde, model, cg = _setup(st, hip_lib, 'vp')
  data, mask, x = _inputs(cfg)
  predict, _ = _updates(st, cfg, sde)
  inpaint = cg.get_pc_inpainter(cfg, sde, **_sampler_args(st, cfg, sde))
  colorize = cg.get_pc_colorizer(cfg, sde, **_sampler_args(st, cfg, sde))
  H = cfg.data.image_size
  bad_masks = [mask.double(), mask[..., :-1], mask.expand(2, 2, H, H).contiguous(), mask * 2., mask - 0.5,
               torch.full_like(mask, float('nan'))]
  for bad in bad_masks:
    with pytest.raises(ValueError):
      inpaint(model, data, bad)
    with pytest.raises(ValueError):
      cg.inpaint_update(predict, sde, model, data, bad, x, 0.5)
  with pytest.raises(ValueError, match='does not match'):
    cg.inpaint_update(predict, sde, model, data[:1], mask, x, 0.5)
  with pytest.raises(ValueError, match='does not match'):
    cg.colorize_update(predict, sde, model, data[:1], x, 0.5)
  with pytest.raises(ValueError, match='3 channels'):
    colorize(model, data[:, :2].contiguous())
  with pytest.raises(ValueError, match='3 channels'):
    cg.decouple(data[:, :2].contiguous())
  # host tensors: the package's device error, nothing computed on the CPU
  for call in (lambda: inpaint(model, data.cpu(), mask), lambda: inpaint(model, data, mask.cpu()),
               lambda: colorize(model, data.cpu()), lambda: cg.inpaint_update(predict, sde, model, data, mask, x.cpu(), 0.5),
               lambda: cg.colorize_update(predict, sde, model, data.cpu(), x, 0.5), lambda: cg.couple(data.cpu())):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      call()
  # the accepted mask forms run: [H,W], [C,H,W], [N,1,H,W], [N,C,H,W]
  for ok in (mask[0, 0], mask[0].expand(3, H, H).contiguous(), mask.expand(2, 1, H, H).contiguous(),
             mask.expand(2, 3, H, H).contiguous()):
    out, _ = cg.inpaint_update(predict, sde, model, data, ok, x, 0.5)
    assert bool(torch.isfinite(out).all())
