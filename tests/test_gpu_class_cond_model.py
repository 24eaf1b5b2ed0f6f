"""The class-conditional network, classifier-free guidance, training and the samplers on the device, against the oracle.

The oracle needs no change: for samples that all carry class c the network equals RefNet with table[c] added to the bias of
the second linear layer of the time MLP.  One such RefNet is built per class present and evaluated on that class's samples;
its gradient of the shifted bias is the reference for row c of the table gradient.  Tiny families vp, rve and wide with
num_classes = 3 and a randomised table, tolerance TOL = 2e-4 of _model_cases."""
import copy

import numpy as np
import pytest
import torch

import ref_torch
from _model_cases import TOL, _inputs
from _model_util import make_state, patched_rng, randomize_, rel_err, tiny_config

pytestmark = pytest.mark.gpu

FAMILIES = ['vp', 'rve', 'wide']
C = 3
_built = {}


def _build(st, lib, family, num_classes=C, zero_table=False, **training):
  """(cfg, cfg_cpu, sde, model, host state_dict) of a tiny network with randomised weights: the weights other than the table
  are the same for every num_classes (randomize_ draws in parameter order, the table is the last parameter)."""
  key = (family, num_classes, zero_table, tuple(training.items()))
  if key in _built:
    return _built[key]
  cfg = tiny_config(st, family)
  if num_classes:
    cfg.model.num_classes = num_classes
  for k, v in training.items():
    cfg.training[k] = v
  cfg.device = torch.device('cuda:0')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  net = net.to(cfg.device)
  randomize_(net, 0)
  if zero_table:
    with torch.no_grad():
      net.class_emb.weight.zero_()
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  model.eval()
  cfg_cpu = copy.deepcopy(cfg)
  cfg_cpu.device = torch.device('cpu')
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  _built[key] = (cfg, cfg_cpu, sde, model, sd)
  return _built[key]


def _bias_key(cfg):
  """The bias of the second linear layer of the time MLP (behind the Fourier projection where there is one)."""
  return f'module.all_modules.{2 if cfg.model.embedding_type == "fourier" else 1}.bias'


def _ref_for(cfg_cpu, sd, c):
  """RefNet of the samples of class c: the unconditional network with table[c] added to that bias."""
  shifted = {k: v.clone() for k, v in sd.items() if k != 'module.class_emb.weight'}
  shifted[_bias_key(cfg_cpu)] += sd['module.class_emb.weight'][c]
  return ref_torch.RefNet(cfg_cpu, shifted)


def _ref_name(key):
  return key[len('module.'):].replace('.', '__')


@pytest.mark.parametrize('family', FAMILIES)
def test_mixed_class_batch_matches_the_per_class_references(st, hip_lib, family):
  mu = st.models.utils
  cfg, cfg_cpu, sde, model, sd = _build(st, hip_lib, family)
  net, dev = model.module, cfg.device
  classes = [1, 1, None, 0]
  rows = [1, 1, C, 0]
  x, t, cond = _inputs(cfg, sde, 4)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  model.zero_grad()
  for p in model.parameters():
    if p.grad is not None:
      p.grad.zero_()
  xg = x.clone().to(dev).requires_grad_(True)
  with mu.class_condition(model, classes):
    y = model(xg, cond.to(dev))
  (y * go.to(dev)).sum().backward()

  yr, gxr, grads, row_grads = torch.zeros_like(x), torch.zeros_like(x), {}, {}
  for c in sorted(set(rows)):
    idx = [i for i, r in enumerate(rows) if r == c]
    ref = _ref_for(cfg_cpu, sd, c).eval()
    xr = x[idx].clone().requires_grad_(True)
    out = ref(xr, cond[idx])
    (out * go[idx]).sum().backward()
    yr[idx], gxr[idx] = out.detach(), xr.grad
    for k, p in ref.named_parameters():
      if p.grad is not None:
        grads[k] = grads.get(k, 0) + p.grad
    row_grads[c] = getattr(ref, _ref_name(_bias_key(cfg))).grad

  assert rel_err(y, yr) <= TOL, f'forward mismatch {rel_err(y, yr):.3e}'
  assert rel_err(xg.grad, gxr) <= TOL, f'input-gradient mismatch {rel_err(xg.grad, gxr):.3e}'
  # parameter gradients, compared as _model_util.grads_close compares them: relative to the tensor's largest entry, but to no
  # less than 1e-3 of the largest gradient entry of the whole model
  scale = max(g.abs().max().item() for g in grads.values())
  for k, p in model.named_parameters():
    if not p.requires_grad or k == 'module.class_emb.weight':
      continue
    g = grads[_ref_name(k)]
    e = (p.grad.detach().cpu() - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * scale)
    assert e <= TOL, f'parameter gradient mismatch {e:.3e} at {k}'
  gtab = net.class_emb.weight.grad.detach().cpu()
  for c, g in row_grads.items():
    e = (gtab[c] - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * scale)
    assert e <= TOL, f'table gradient mismatch {e:.3e} at row {c}'
  assert not gtab[2].any(), 'the row of the absent class received a gradient'


@pytest.mark.parametrize('family', FAMILIES)
def test_fresh_zero_table_model_equals_the_unconditional_one(st, hip_lib, family):
  mu = st.models.utils
  cfg, _, sde, model, sd = _build(st, hip_lib, family, zero_table=True)
  _, _, _, plain, sd0 = _build(st, hip_lib, family, num_classes=0)
  assert list(sd) == list(sd0) + ['module.class_emb.weight'] and all(torch.equal(sd[k], sd0[k]) for k in sd0)
  x, t, cond = _inputs(cfg, sde, 4)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  with torch.no_grad():
    want = plain(x, cond)
    assert torch.equal(model(x, cond), want)
    with mu.class_condition(model, [0, 1, 2, None]):
      assert torch.equal(model(x, cond), want)


@pytest.mark.parametrize('family', FAMILIES)
def test_guidance(st, hip_lib, family):
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, family)
  dev = cfg.device
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(dev), cond.to(dev)
  y = torch.tensor([2, 0, 3])
  with torch.no_grad():
    with mu.class_condition(model, y):
      c = model(x, cond)
    with mu.class_condition(model, y, guidance=0.0):
      assert torch.equal(model(x, cond), c)
    with mu.class_condition(model, [None] * 3):
      u = model(x, cond)
    assert torch.equal(model(x, cond), u), 'no classes given: every sample takes the null row'
    assert rel_err(c, u) > 100 * TOL, 'the classes do not reach the output'
    with mu.class_condition(model, y, guidance=1.5):
      g = model(x, cond)
    assert rel_err(g, c + 1.5 * (c - u)) <= TOL, f'guided evaluation off by {rel_err(g, c + 1.5 * (c - u)):.3e}'
    with mu.class_condition(model, y, guidance=-1.0):
      n = model(x, cond)
    assert rel_err(n, u) <= TOL, f'guidance -1 off the null evaluation by {rel_err(n, u):.3e}'
    with mu.precision(model, 'fp16'), mu.class_condition(model, y, guidance=1.5):
      h = model(x, cond)
    assert h.shape == x.shape and bool(torch.isfinite(h).all())
  # the input gradient under grad mode: the combination is written with torch operators there
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
  xg = x.clone().requires_grad_(True)
  with mu.class_condition(model, y, guidance=1.5):
    out = model(xg, cond)
  assert rel_err(out, g) <= TOL
  gx, = torch.autograd.grad((out * go).sum(), xg)
  xs = x.clone().requires_grad_(True)
  with mu.class_condition(model, y):
    cs = model(xs, cond)
  with mu.class_condition(model, [None] * 3):
    us = model(xs, cond)
  want, = torch.autograd.grad(((cs + 1.5 * (cs - us)) * go).sum(), xs)
  assert rel_err(gx, want) <= TOL, f'guided input gradient off by {rel_err(gx, want):.3e}'


def test_input_only_backward_leaves_the_table_gradient(st, hip_lib):
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp')
  net = model.module
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  net.engine().ensure_flat()
  grad = net.class_emb.weight.grad
  grad.fill_(7.0)
  for _ in range(2):              # the second call replays the captured backward
    xg = x.clone().requires_grad_(True)
    with mu.class_condition(model, [0, 1, 1]):
      out = model(xg, cond)
    gx, = torch.autograd.grad(out.sum(), xg)
    assert bool(torch.isfinite(gx).all()) and net.class_emb.weight.grad is grad
    assert bool((grad == 7.0).all()), 'an input-only backward wrote the table gradient'
  xg = x.clone().requires_grad_(True)
  with mu.class_condition(model, [0, 1, 1]):
    model(xg, cond).sum().backward()
  g = net.class_emb.weight.grad
  assert bool((g[0] != 7.0).any()) and bool((g[1] != 7.0).any()) and bool((g[2:] == 7.0).all())
  model.zero_grad()


@pytest.mark.parametrize('family', FAMILIES)
def test_training_step_against_the_shifted_reference(st, hip_lib, family):
  """One step of step_fn, class_dropout = 0, every sample of class 1, against the reference step on the bias-shifted RefNet.
  The table row and the bias receive the same gradient, so the row moves as the reference's shifted bias does."""
  base = tiny_config(st, family)
  base.model.num_classes = C
  base.training.class_dropout = 0.0
  base.optim.warmup = 0
  assert base.optim.weight_decay == 0
  cfg, cfg_cpu = copy.deepcopy(base), copy.deepcopy(base)
  cfg.device, cfg_cpu.device = torch.device('cuda:0'), torch.device('cpu')
  sde = st.sde_lib.get_sde(cfg, None)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(hip_lib)
  net = net.to(cfg.device)
  randomize_(net, 0)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  ref = st.models.utils.DataParallel(_ref_for(cfg_cpu, sd, 1))
  state = make_state(st, cfg, model)
  assert type(state['optimizer']).__name__ == 'FusedAdam'
  state['optimizer']._backend = hip_lib
  state['ema'].set_backend(hip_lib)
  rstate = make_state(st, cfg_cpu, ref)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  rstep_fn = st.losses.get_step_fn(cfg_cpu, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg_cpu))
  B = 4
  batch = st.datasets.synthetic_batch(cfg_cpu, B, generator=torch.Generator().manual_seed(100))
  np.random.seed(7)
  with patched_rng(50):
    loss = step_fn(state, batch.to(cfg.device), torch.ones(B, dtype=torch.int64, device=cfg.device))
  np.random.seed(7)
  with patched_rng(50):
    rloss = rstep_fn(rstate, batch)
  assert loss.shape == rloss.shape and rel_err(loss, rloss) <= TOL, f'loss mismatch {rel_err(loss, rloss):.3e}'
  lr = cfg.optim.lr
  table0, table1 = sd['module.class_emb.weight'], net.class_emb.weight.detach().cpu()
  rbias0 = sd[_bias_key(cfg)] + table0[1]
  rbias1 = getattr(ref.module, _ref_name(_bias_key(cfg))).detach()
  moved = (rbias1 - rbias0).abs().max().item()
  assert moved > 0.5 * lr, f'the reference bias moved by {moved:.3e} only: the step updates nothing'
  d = ((table1[1] - table0[1]) - (rbias1 - rbias0)).abs().max().item()
  assert d <= 0.05 * lr + 1e-7, f'table row 1 drifts {d:.3e} from the reference update'
  for c in (0, 2, 3):
    assert torch.equal(table1[c], table0[c]), f'row {c} of an absent class changed'


def _sampler(st, cfg, sde, n_steps, **options):
  c = copy.deepcopy(cfg)
  for k, v in options.items():
    setattr(c.sampling, k, v)
  shape = (2, c.data.num_channels, c.data.image_size, c.data.image_size)
  s = copy.deepcopy(sde)
  if n_steps is not None:
    s.N = n_steps
  return st.sampling.get_sampling_fn(c, s, shape, st.datasets.get_data_inverse_scaler(c), 1e-3), shape


@pytest.mark.parametrize('method', ['pc', 'dpm_solver'])
def test_samplers_take_classes_through_the_context(st, hip_lib, method):
  mu = st.models.utils
  if method == 'pc':
    options, n = dict(method='pc', predictor='euler_maruyama', corrector='none'), 4
  else:
    options, n = dict(method='dpm_solver', dpm_steps=3, noise_removal=True), None
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp')
  fn, shape = _sampler(st, cfg, sde, n, **options)

  def run(m, *context):
    torch.manual_seed(3)
    if not context:
      return fn(m)[0]
    with mu.class_condition(m, *context):
      return fn(m)[0]

  guided, plain = run(model, [0, 2], 1.5), run(model, [0, 2], 0.0)
  for out in (guided, plain):
    assert out.shape == shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
  assert not torch.equal(guided, plain), 'guidance does not reach the sampler'
  assert torch.equal(run(model, [0, 2], 1.5), guided), 'two guided runs under one seed differ'
  # all-null classes on the zero-table model: the unconditional run, bit for bit
  _, _, _, zero, _ = _build(st, hip_lib, 'vp', zero_table=True)
  _, _, _, uncond, _ = _build(st, hip_lib, 'vp', num_classes=0)
  assert torch.equal(run(zero, [None, None], 0.0), run(uncond))
