"""The fp16 training mode end to end (Executor.training_precision, models.utils.training_precision,
config.training.precision) on the device.

Gradient agreement is the relative norm ||g16 - g32|| / max(||g32||, 1e-3 G) per parameter tensor, G = the largest ||g32|| of
the model: the floor keeps out tensors whose gradient is zero in exact arithmetic and only round-off in fp32 (the key bias of
attention: softmax is invariant to it, so its fp32 gradient is ~1e-7 of the others').  The loss-curve agreement is
max_i |l16_i - l32_i| / max_i |l32_i| over the batch-mean curve.  The bounds carry a margin of about 4x over the values
measured on an MI355X, which are given next to each bound.  Sample quality and NLL of models trained in this mode are not
measured anywhere in this suite.
"""
from importlib import import_module

import numpy as np
import pytest
import torch

from _fullsize_cases import build_full
from _launch_trace import LibProxy
from _model_util import build_pair, make_state, patched_rng, tiny_config

pytestmark = pytest.mark.gpu

# ||g16 - g32|| / max(||g32||, 1e-3 G), worst parameter tensor, bounds ~4x the MI355X measurement: tiny net (nf 96) 4.1e-4
# (median 2.1e-4), full-size DDPM++ CIFAR-10 at batch 16 6.1e-3 (median 7.2e-4; the per-layer contraction error is ~3e-4, and
# it compounds through the ~30 layers a deep gradient passes)
GRAD_RTOL = {'wide': 2e-3, 'cifar10': 2.5e-2}
# fp16 vs fp32 batch-mean loss curve over 50 steps of the tiny VP net: measured 8.3e-6 (plain), 9.7e-6 (2 micro-batches,
# training.mixed)
CURVE_RTOL = 4e-5
TWINS = {'conv2d_fwd_pl_f16x1', 'conv2d_fwd_rec_f16x1', 'conv2d_fwd_wp_f16x1', 'conv2d_dgrad_pl_f16x1',
         'conv2d_dgrad_rec_f16x1', 'conv2d_dgrad_wp_f16x1', 'conv2d_wgrad_pl_f16x1', 'conv2d_wgrad_pl_wgs_f16x1',
         'conv2d_wgrad_amax_f16x1'}


def _wide(st, lib, micro=1, mixed=False):
  cfg = tiny_config(st, 'wide')
  cfg.optim.warmup = 10
  cfg.optim.num_micro_batch = micro
  cfg.training.mixed = mixed
  return build_pair(st, cfg, lib)


def _train(st, lib, precision, steps, B=8, micro=1, mixed=False):
  """`steps` step_fn calls on a fresh tiny VP net; precision None = no key in the config"""
  cfg, _, sde, model, _ = _wide(st, lib, micro, mixed)
  if precision is not None:
    cfg.training.precision = precision
  state = make_state(st, cfg, model)
  state['optimizer']._backend = lib
  state['ema'].set_backend(lib)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  losses = []
  for i in range(steps):
    batch = st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(1000 + i))
    np.random.seed(70 + i)
    with patched_rng(500 + i):
      losses.append(step_fn(state, batch.to(cfg.device)).clone())
  torch.cuda.synchronize()
  params = [p.detach().clone() for p in model.parameters()]
  ema = [s.detach().clone() for s in state['ema'].shadow_params]
  return torch.stack(losses), params, ema, model


def _same_run(a, b):
  assert torch.equal(a[0], b[0]), 'losses differ'
  assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])), 'parameters differ'
  assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])), 'EMA differs'


def test_absent_key_is_bitwise_fp32(st, hip_lib):
  a = _train(st, hip_lib, None, 3)
  b = _train(st, hip_lib, 'fp32', 3)
  _same_run(a, b)


def test_fp16_step_calls_the_twins_in_every_direction(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  ex = model.module.engine()
  ex.profiler, saved = import_module(st.__name__ + '.engine.profile').KernelTimer(), ex.profiler
  try:
    x = torch.randn(4, 3, 16, 16, device=cfg.device)
    t = torch.full((4,), 0.5, device=cfg.device)
    with st.models.utils.training_precision(model, 'fp16'):
      model.train()
      model(x, t).square().sum().backward()
    torch.cuda.synchronize()
    labels = [r[0] for r in ex.profiler.records]
  finally:
    ex.profiler = saved
  f16 = [k for k in labels if k.endswith('.f16')]
  for direction in ('.fwd.', '.dgrad.', '.wgrad.'):
    assert any(direction in k for k in f16), (direction, sorted(set(labels)))
  # no split-form convolution stayed on fp32: every conv x2 label carries .f16 (attention stays fp32-equivalent)
  assert not [k for k in labels if k.startswith('conv') and '.x2' in k and not k.endswith('.f16')], sorted(set(labels))
  print('  labels:', sorted(set(f16)))


def test_fp16_step_calls_only_twins_for_split_forms(st, hip_lib):
  """with the side stream on (no profiler): every split-form library call of a training step is a twin"""
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  ex = model.module.engine()
  assert ex.use_side
  calls = []

  ex.use_graphs, saved = False, ex.use_graphs
  ex.lib = LibProxy(st.engine.lib, hip_lib, calls, execute=True)
  try:
    x = torch.randn(4, 3, 16, 16, device=cfg.device)
    t = torch.full((4,), 0.5, device=cfg.device)
    model.train()
    with st.models.utils.training_precision(model, 'fp16'):
      model(x, t).square().sum().backward()
  finally:
    ex.lib, ex.use_graphs = hip_lib, saved
  torch.cuda.synchronize()
  log = [n for n, _ in calls]
  used = set(log) & TWINS
  assert {'conv2d_fwd_pl_f16x1', 'conv2d_dgrad_pl_f16x1'} <= used, sorted(set(log))
  assert used & {'conv2d_wgrad_pl_f16x1', 'conv2d_wgrad_pl_wgs_f16x1'}, sorted(set(log))
  # every backward contraction goes through a twin (non-split forms run inside it as in fp32); plane forwards too
  assert not {n for n in log if n.startswith(('conv2d_dgrad', 'conv2d_wgrad')) and n.endswith('_f32')}, sorted(set(log))
  assert 'conv2d_fwd_pl_f32' not in log


def test_fp16_runs_repeat_bitwise(st, hip_lib):
  a = _train(st, hip_lib, 'fp16', 3)
  b = _train(st, hip_lib, 'fp16', 3)
  assert a[3].module.engine().use_side
  _same_run(a, b)
  c = _train(st, hip_lib, 'fp32', 3)
  assert not torch.equal(a[0], c[0]), 'the fp16 mode changed nothing'


def _grads(st, model, x, t, precision):
  model.zero_grad(set_to_none=True)
  model.train()
  with st.models.utils.training_precision(model, precision):
    model(x, t).square().mean().backward()
  torch.cuda.synchronize()
  return {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}


def _grad_agreement(st, label, model, cfg, B, H):
  g = torch.Generator().manual_seed(3)
  x = torch.randn(B, cfg.data.num_channels, H, H, generator=g).to(cfg.device)
  t = (torch.rand(B, generator=g) * 0.9 + 0.05).to(cfg.device) * 999
  g32 = _grads(st, model, x, t, 'fp32')
  g16 = _grads(st, model, x, t, 'fp16')
  floor = 1e-3 * max(a.norm().item() for a in g32.values())
  errs = {k: (g16[k] - a).norm().item() / max(a.norm().item(), floor) for k, a in g32.items()}
  wk = max(errs, key=errs.get)
  worst = errs[wk]
  print(f'  {label}: ||g16 - g32|| / max(||g32||, 1e-3 G) over {len(errs)} tensors: worst {worst:.3e} ({wk}), median '
        f'{np.median(list(errs.values())):.3e}')
  return worst, wk


def test_gradients_agree_tiny(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  worst, wk = _grad_agreement(st, 'wide', model, cfg, 8, 16)
  assert worst <= GRAD_RTOL['wide'], (worst, wk)


def test_gradients_agree_cifar10(st, hip_lib):
  cfg, _, sde, model, _ = build_full(st, 'cifar10_ddpmpp_nll_st', hip_lib)
  worst, wk = _grad_agreement(st, 'cifar10', model, cfg, 16, cfg.data.image_size)
  assert worst <= GRAD_RTOL['cifar10'], (worst, wk)


@pytest.mark.parametrize('micro,mixed', [(1, False), (2, True)], ids=['plain', 'micro2_mixed'])
def test_loss_curve_tracks_fp32(st, hip_lib, micro, mixed):
  l32, p32, _, _ = _train(st, hip_lib, 'fp32', 50, micro=micro, mixed=mixed)
  l16, p16, _, _ = _train(st, hip_lib, 'fp16', 50, micro=micro, mixed=mixed)
  c32, c16 = l32.double().mean(1), l16.double().mean(1)
  err = ((c16 - c32).abs().max() / c32.abs().max()).item()
  print(f'  curve ({micro} micro-batches, mixed={mixed}): fp32 {c32[0]:.4f} -> {c32[-1]:.4f}, fp16 {c16[0]:.4f} -> '
        f'{c16[-1]:.4f}, max rel. difference {err:.3e}')
  assert torch.isfinite(l16).all()
  assert err <= CURVE_RTOL, err


def test_scope_and_refusals(st, hip_lib):
  cfg, _, sde, model, _ = _wide(st, hip_lib)
  mu = st.models.utils
  x = torch.randn(2, 3, 16, 16, device=cfg.device)
  t = torch.full((2,), 0.5, device=cfg.device)
  # precision('fp16') alone still refuses a training forward
  with mu.precision(model, 'fp16'):
    model.train()
    with pytest.raises(ValueError, match='forward-only'):
      model(x, t)
  # a no-grad forward inside training_precision('fp16') is the fp32 one, bit for bit (train and eval mode)
  for train in (True, False):
    model.train(train)
    with torch.no_grad():
      y32 = model(x, t)
      with mu.training_precision(model, 'fp16'):
        y = model(x, t)
    assert torch.equal(y, y32)
  # ... while a no-grad forward inside both contexts follows precision()
  model.eval()
  with torch.no_grad(), mu.training_precision(model, 'fp16'), mu.precision(model, 'fp16'):
    y16 = model(x, t)
  assert not torch.equal(y16, y32)
  # the likelihood refuses to run inside the training mode
  inv = st.datasets.get_data_inverse_scaler(cfg)
  lfn = st.likelihood.get_likelihood_fn(cfg, sde, inv)
  with mu.training_precision(model, 'fp16'), pytest.raises(ValueError, match='fp32 only'):
    lfn(model, torch.rand(2, 3, 16, 16, device=cfg.device))
