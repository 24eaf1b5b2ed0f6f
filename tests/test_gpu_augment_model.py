"""The augmentation embedding in the network, training under augmentation and sampling on the device, against the oracle.

The oracle needs no change: for ONE sample with labels l the network equals RefNet with W l added to the bias of the second
linear layer of the time MLP -- temb += labels @ W.T at the place engine.graph.AugmentEmbedding adds it.  One such RefNet is
built per sample; its gradient of the shifted bias g_b gives the reference of the weight gradient, sum_b outer(g_b, l_b).
Tiny families with augment_dim = 9, tolerance TOL = 2e-4 of _model_cases (the model-level bar of every parity test)."""
import copy

import numpy as np
import pytest
import torch

import ref_torch
from _model_cases import TOL, _inputs
from _model_util import make_state, patched_rng, randomize_, rel_err, tiny_config

pytestmark = pytest.mark.gpu

FAMILIES = ['vp', 'rve']
K = 9
_built = {}


def _build(st, lib, family, augment_dim=K, num_classes=0, zero_weight=False):
  """(cfg, cfg_cpu, sde, model, host state_dict) of a tiny network with randomised weights: the weights other than the
  embedding's are the same for every augment_dim (randomize_ draws in parameter order, the embedding is the last parameter)."""
  key = (family, augment_dim, num_classes, zero_weight)
  if key in _built:
    return _built[key]
  cfg = tiny_config(st, family)
  if augment_dim:
    cfg.model.augment_dim = augment_dim
  if num_classes:
    cfg.model.num_classes = num_classes
  cfg.device = torch.device('cuda:0')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  net = net.to(cfg.device)
  randomize_(net, 0)
  if zero_weight:
    with torch.no_grad():
      net.augment_emb.weight.zero_()
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  model.eval()
  cfg_cpu = copy.deepcopy(cfg)
  cfg_cpu.device = torch.device('cpu')
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  _built[key] = (cfg, cfg_cpu, sde, model, sd)
  return _built[key]


def _labels(B, seed=3):
  g = torch.Generator().manual_seed(seed)
  l = torch.randn(B, K, generator=g)
  l[torch.rand(B, K, generator=g) < 0.3] = 0.0
  return l


def _bias_key(cfg):
  return f'module.all_modules.{2 if cfg.model.embedding_type == "fourier" else 1}.bias'


def _ref_name(key):
  return key[len('module.'):].replace('.', '__')


def _ref_for(cfg_cpu, sd, label_row):
  shifted = {k: v.clone() for k, v in sd.items() if k != 'module.augment_emb.weight'}
  shifted[_bias_key(cfg_cpu)] += sd['module.augment_emb.weight'] @ label_row
  return ref_torch.RefNet(cfg_cpu, shifted)


@pytest.mark.parametrize('family', FAMILIES)
def test_zero_weight_or_zero_labels_equal_the_plain_network(st, hip_lib, family):
  mu = st.models.utils
  cfg, _, sde, zero, sdz = _build(st, hip_lib, family, zero_weight=True)
  _, _, _, rand, sdr = _build(st, hip_lib, family)
  _, _, _, plain, sd0 = _build(st, hip_lib, family, augment_dim=0)
  assert list(sdr) == list(sd0) + ['module.augment_emb.weight'] and all(torch.equal(sdr[k], sd0[k]) for k in sd0)
  assert sdr['module.augment_emb.weight'].any() and not sdz['module.augment_emb.weight'].any()
  x, t, cond = _inputs(cfg, sde, 4)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  labels = _labels(4)
  with torch.no_grad():
    want = plain(x, cond)
    assert torch.equal(zero(x, cond), want)
    with mu.augment_condition(zero, labels):
      assert torch.equal(zero(x, cond), want), 'a zero weight lets the labels through'
    assert torch.equal(rand(x, cond), want), 'no labels in force: zeros'
    with mu.augment_condition(rand, torch.zeros(4, K)):
      assert torch.equal(rand(x, cond), want)
    with mu.augment_condition(rand, labels):
      assert rel_err(rand(x, cond), want) > 100 * TOL, 'the labels do not reach the output'


@pytest.mark.parametrize('family', FAMILIES)
def test_random_weight_and_labels_match_the_per_sample_references(st, hip_lib, family):
  mu = st.models.utils
  cfg, cfg_cpu, sde, model, sd = _build(st, hip_lib, family)
  net, dev = model.module, cfg.device
  B = 3
  labels = _labels(B)
  x, t, cond = _inputs(cfg, sde, B)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  model.zero_grad()
  for p in model.parameters():
    if p.grad is not None:
      p.grad.zero_()
  xg = x.clone().to(dev).requires_grad_(True)
  with mu.augment_condition(model, labels):
    y = model(xg, cond.to(dev))
  (y * go.to(dev)).sum().backward()

  yr, gxr, grads = torch.zeros_like(x), torch.zeros_like(x), {}
  gw = torch.zeros_like(sd['module.augment_emb.weight'])
  for b in range(B):
    ref = _ref_for(cfg_cpu, sd, labels[b]).eval()
    xr = x[b:b + 1].clone().requires_grad_(True)
    out = ref(xr, cond[b:b + 1])
    (out * go[b:b + 1]).sum().backward()
    yr[b:b + 1], gxr[b:b + 1] = out.detach(), xr.grad
    for k, p in ref.named_parameters():
      if p.grad is not None:
        grads[k] = grads.get(k, 0) + p.grad
    gw += torch.outer(getattr(ref, _ref_name(_bias_key(cfg))).grad, labels[b])

  assert rel_err(y, yr) <= TOL, f'forward mismatch {rel_err(y, yr):.3e}'
  assert rel_err(xg.grad, gxr) <= TOL, f'input-gradient mismatch {rel_err(xg.grad, gxr):.3e}'
  scale = max(g.abs().max().item() for g in grads.values())
  for k, p in model.named_parameters():
    if not p.requires_grad or k == 'module.augment_emb.weight':
      continue
    g = grads[_ref_name(k)]
    e = (p.grad.detach().cpu() - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * scale)
    assert e <= TOL, f'parameter gradient mismatch {e:.3e} at {k}'
  got = net.augment_emb.weight.grad.detach().cpu()
  e = (got - gw).abs().max().item() / max(gw.abs().max().item(), 1e-3 * scale)
  assert gw.abs().max().item() > 0 and e <= TOL, f'weight gradient mismatch {e:.3e}'
  model.zero_grad()


def test_input_only_backward_leaves_the_weight_gradient(st, hip_lib):
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp')
  net = model.module
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  labels = _labels(3)
  net.engine().ensure_flat()
  grad = net.augment_emb.weight.grad
  grad.fill_(7.0)
  for _ in range(2):              # the second call replays the captured backward
    xg = x.clone().requires_grad_(True)
    with mu.augment_condition(model, labels):
      out = model(xg, cond)
    gx, = torch.autograd.grad(out.sum(), xg)
    assert bool(torch.isfinite(gx).all()) and net.augment_emb.weight.grad is grad
    assert bool((grad == 7.0).all()), 'an input-only backward wrote the weight gradient'
  xg = x.clone().requires_grad_(True)
  with mu.augment_condition(model, labels):
    model(xg, cond).sum().backward()
  assert bool((net.augment_emb.weight.grad != 7.0).any())
  model.zero_grad()


def _train_config(st, loss):
  base = tiny_config(st, 'vp')
  if loss == 'edm':
    base = st.configs.edm(base)
  elif loss == 'consistency':
    base = st.configs.consistency(base)
  base.training.augment = 0.5
  base.model.augment_dim = K
  base.optim.warmup = 0
  base.seed = 13
  base.device = torch.device('cuda:0')
  return base


@pytest.mark.parametrize('loss', ['sm', 'edm', 'consistency'])
def test_three_training_steps_under_augmentation(st, hip_lib, loss):
  cfg = _train_config(st, loss)
  sde = st.sde_lib.get_sde(cfg, None)

  def run():
    torch.manual_seed(0)
    net = st.models.ncsnpp.NCSNpp(cfg, sde)
    net.set_backend(hip_lib)
    net = net.to(cfg.device)
    randomize_(net, 0)
    with torch.no_grad():
      net.augment_emb.weight.zero_()                 # as a fresh network has it
    model = st.models.utils.DataParallel(net)
    net.engine().ensure_flat()
    state = make_state(st, cfg, model)
    state['optimizer']._backend = hip_lib
    state['ema'].set_backend(hip_lib)
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    losses = []
    for i in range(3):
      batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(100 + i)).to(cfg.device)
      np.random.seed(7 + i)
      with patched_rng(50 + i):
        losses.append(step_fn(state, batch))
    assert net._aug_ctx is None
    return torch.stack(losses), net.augment_emb.weight.detach().cpu().clone()

  l1, w1 = run()
  l2, w2 = run()
  assert l1.shape == (3, 4) and bool(torch.isfinite(l1).all())
  assert torch.equal(l1, l2) and torch.equal(w1, w2), 'two runs of the same three steps differ'
  assert bool(torch.isfinite(w1).all()) and w1.abs().max().item() > 0, 'augment_emb.weight was not updated'


def test_guided_evaluation_repeats_the_labels(st, hip_lib):
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp', num_classes=3)
  with torch.no_grad():                                # randomize_ gave the class rows values; the embedding too
    assert model.module.class_emb.weight.any() and model.module.augment_emb.weight.any()
  dev = cfg.device
  B = 3
  x, t, cond = _inputs(cfg, sde, B)
  x, cond = x.to(dev), cond.to(dev)
  labels = _labels(B)
  y = torch.tensor([2, 0, 3])
  with torch.no_grad():
    with mu.augment_condition(model, labels):
      with mu.class_condition(model, y):
        c = model(x, cond)
      with mu.class_condition(model, [None] * B):
        u = model(x, cond)
      with mu.class_condition(model, y, guidance=1.5):
        g = model(x, cond)
    with mu.class_condition(model, y, guidance=1.5):
      g0 = model(x, cond)
    with mu.class_condition(model, y, guidance=1.5), mu.augment_condition(model, labels):
      g2 = model(x, cond)
  want = c + 1.5 * (c - u)
  assert rel_err(g, want) <= TOL, f'guided evaluation off by {rel_err(g, want):.3e}'
  assert torch.equal(g2, g)
  assert rel_err(g0, g) > 100 * TOL, 'the labels do not reach the guided evaluation'
  assert rel_err(c, u) > 100 * TOL


def test_a_sampler_evaluates_with_zero_labels(st, hip_lib):
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp')
  c = copy.deepcopy(cfg)
  c.sampling.method, c.sampling.predictor, c.sampling.corrector = 'pc', 'euler_maruyama', 'none'
  s = copy.deepcopy(sde)
  s.N = 4
  shape = (2, c.data.num_channels, c.data.image_size, c.data.image_size)
  fn = st.sampling.get_sampling_fn(c, s, shape, st.datasets.get_data_inverse_scaler(c), 1e-3)
  torch.manual_seed(3)
  plain = fn(model)[0]
  torch.manual_seed(3)
  with mu.augment_condition(model, torch.zeros(2, K)):
    zeros = fn(model)[0]
  torch.manual_seed(3)
  with mu.augment_condition(model, _labels(2)):
    told = fn(model)[0]
  assert plain.shape == shape and bool(torch.isfinite(plain).all())
  assert torch.equal(plain, zeros), 'a sampler without labels is not the evaluation with zero labels'
  assert not torch.equal(plain, told)
