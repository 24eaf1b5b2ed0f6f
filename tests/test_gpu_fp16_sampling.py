"""The fp16 mode end to end (engine precision, config.sampling.precision, models.utils.precision) on the device.

Score agreement is max|s16 - s32| / max|s32| over a batch; the bounds carry a 4x margin over the values measured on an
MI355X, which are given next to each bound.  Sample quality (FID) of the mode is not measured anywhere in this suite.
"""
import copy

import pytest
import torch

from _fullsize_cases import build_full
from _launch_trace import LibProxy
from _model_util import build_pair, patched_rng, tiny_config

pytestmark = pytest.mark.gpu

# max|s16 - s32| / max|s32|, bounds >= 4x the MI355X measurement: tiny DDPM++ (nf 96) 1.19e-4 (VP) / 1.30e-4 (VE), full-size
# DDPM++ CIFAR-10 at batch 16 8.94e-4 (VP) / 1.35e-3 (VE)
SCORE_RTOL = {'wide-vp': 5e-4, 'wide-ve': 6e-4, 'cifar10-vp': 4e-3, 'cifar10-ve': 6e-3}
PC_RTOL = 1e-4             # 6-step PC run on the tiny net, max|x16 - x32| / max|x32|: measured 2.43e-5


def _wide(st, lib, sde_name='vpsde'):
  cfg = tiny_config(st, 'wide')
  cfg.training.sde = sde_name
  if sde_name == 'vesde':
    cfg.training.continuous = True
  return build_pair(st, cfg, lib)


def _pc(cfg, family_predictor='euler_maruyama', corrector='none'):
  cfg = copy.deepcopy(cfg)
  cfg.sampling.method, cfg.sampling.predictor, cfg.sampling.corrector = 'pc', family_predictor, corrector
  return cfg


def _sample(st, cfg, sde, model, precision, n=4, seed=11):
  c = copy.deepcopy(cfg)
  if precision is not None:
    c.sampling.precision = precision
  shape = (4, c.data.num_channels, c.data.image_size, c.data.image_size)
  fn = st.sampling.get_sampling_fn(c, sde, shape, st.datasets.get_data_inverse_scaler(c), 1e-3)
  with patched_rng(seed):
    return fn(model)


def test_default_precision_is_bitwise_fp32(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  cfg = _pc(cfg)
  sde.N = 4
  assert 'precision' not in cfg.sampling
  x0, n0 = _sample(st, cfg, sde, model, None)
  x1, n1 = _sample(st, cfg, sde, model, 'fp32')
  torch.cuda.synchronize()
  assert n0 == n1 and torch.equal(x0, x1)


def test_fp16_evaluation_calls_the_twins(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  ex = model.module.engine()
  x = torch.randn(4, 3, 16, 16, device=cfg.device)
  t = torch.full((4,), 0.5, device=cfg.device)
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=True)
  calls = []

  ex.use_graphs, saved = False, ex.use_graphs          # eager launches: every call goes through the handle
  ex.lib = LibProxy(st.engine.lib, hip_lib, calls, execute=True)
  try:
    with torch.no_grad():
      score_fn(x, t)
      f32 = [n for n, _ in calls]
      del calls[:]
      with st.models.utils.precision(model, 'fp16'):
        score_fn(x, t)
      f16 = [n for n, _ in calls]
  finally:
    ex.lib, ex.use_graphs = hip_lib, saved
  torch.cuda.synchronize()
  twins = {'conv2d_fwd_pl_f16x1', 'conv2d_fwd_rec_f16x1', 'conv2d_fwd_wp_f16x1'}
  assert not twins & set(f32)
  used = [n for n in f16 if n in twins]
  assert 'conv2d_fwd_pl_f16x1' in used, sorted(set(f16))
  assert not {'conv2d_fwd_pl_f32'} & set(f16), 'a split-form forward stayed on fp32 in the fp16 mode'
  # every fp32 split-form call of the fp32 evaluation became a twin call
  n32 = sum(f32.count(n) for n in ('conv2d_fwd_pl_f32', 'conv2d_fwd_rec_f32', 'conv2d_fwd_wp_f32'))
  assert len(used) + sum(f16.count(n) for n in ('conv2d_fwd_rec_f32', 'conv2d_fwd_wp_f32')) == n32


def _score_err(st, cfg, sde, model, B=8, seed=3):
  g = torch.Generator().manual_seed(seed)
  S = cfg.data.image_size
  x = torch.randn(B, cfg.data.num_channels, S, S, generator=g).to(cfg.device)
  t = (torch.rand(B, generator=g) * 0.9 + 0.05).to(cfg.device)
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=True)
  with torch.no_grad():
    s32 = score_fn(x, t)
    with st.models.utils.precision(model, 'fp16'):
      s16 = score_fn(x, t)
      s16b = score_fn(x, t)                    # second call: the fp16 program's hipGraph replay
    s32b = score_fn(x, t)
  torch.cuda.synchronize()
  assert torch.equal(s16, s16b) and torch.equal(s32, s32b), 'modes share state: a replay changed the result'
  assert torch.isfinite(s16).all()
  return ((s16 - s32).abs().max() / s32.abs().max()).item()


@pytest.mark.parametrize('sde_name', ['vpsde', 'vesde'])
def test_score_agreement_tiny(st, hip_lib, sde_name):
  cfg, _, sde, model, _ = _wide(st, hip_lib, sde_name)
  key = 'wide-' + sde_name[:2]
  e = _score_err(st, cfg, sde, model)
  print(f'  {key}: max|s16 - s32| / max|s32| = {e:.3e} (bound {SCORE_RTOL[key]:.0e})')
  assert 0 < e <= SCORE_RTOL[key]


@pytest.mark.parametrize('sde_name', ['vpsde', 'vesde'])
def test_score_agreement_cifar10(st, hip_lib, sde_name):
  cfg, _, sde, model, _ = build_full(st, 'cifar10_ddpmpp_nll_st', hip_lib)
  if sde_name == 'vesde':
    cfg.training.sde = 'vesde'
    sde = st.sde_lib.get_sde(cfg, None)
  key = 'cifar10-' + sde_name[:2]
  e = _score_err(st, cfg, sde, model, B=16)
  print(f'  {key}: max|s16 - s32| / max|s32| = {e:.3e} (bound {SCORE_RTOL[key]:.0e})')
  assert 0 < e <= SCORE_RTOL[key]


def test_short_fp16_pc_run(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  cfg = _pc(cfg)
  sde.N = 6
  x32, n32 = _sample(st, cfg, sde, model, 'fp32')
  x16, n16 = _sample(st, cfg, sde, model, 'fp16')
  torch.cuda.synchronize()
  assert n16 == n32
  assert torch.isfinite(x16).all()
  e = ((x16 - x32).abs().max() / x32.abs().max()).item()
  print(f'  PC N = 6: max|x16 - x32| / max|x32| = {e:.3e} (bound {PC_RTOL:.0e})')
  assert 0 < e <= PC_RTOL


def test_refusals(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  x = torch.randn(2, 3, 16, 16, device=cfg.device)
  t = torch.full((2,), 0.5, device=cfg.device)
  mu = st.models.utils
  with mu.precision(model, 'fp16'):
    model.train()                                         # a training forward
    with pytest.raises(ValueError, match='forward-only'):
      model(x, t)
    model.eval()
    # need_xgrad: a forward whose input gradient is asked for
    with pytest.raises(ValueError, match='forward-only'):
      model(x.clone().requires_grad_(True), t)
    # grad mode at all (a backward may follow)
    with torch.enable_grad(), pytest.raises(ValueError, match='forward-only'):
      model(x, t)
    with torch.no_grad():
      assert torch.isfinite(model(x, t)).all()            # the forward-only evaluation itself runs
  # ODE sampler and likelihood with an fp16 config
  c = copy.deepcopy(cfg)
  c.sampling.method, c.sampling.precision = 'ode', 'fp16'
  inv = st.datasets.get_data_inverse_scaler(c)
  with pytest.raises(ValueError, match='ODE'):
    st.sampling.get_sampling_fn(c, sde, (2, 3, 16, 16), inv, 1e-3)
  with pytest.raises(ValueError, match='fp32 only'):
    st.likelihood.get_likelihood_fn(c, sde, inv)
  # likelihood inside the mode: its divergence differentiates the network
  lfn = st.likelihood.get_likelihood_fn(cfg, sde, inv)
  with mu.precision(model, 'fp16'), pytest.raises(ValueError, match='forward-only'):
    lfn(model, torch.rand(2, 3, 16, 16, device=cfg.device))
